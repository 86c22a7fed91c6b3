"""Training-path utilities (reference: gans/utils.py:21-42, 85-105, 238-271) and the visualisation helpers a latent
walk and the training log need: cycle, colorize, points_to_normal_2d, power_spectrum_2d (utils.py:136-138, 167-209).
The rest of the reference file's visualisation code (the video writers) is out of scope."""
import os
import random

import numpy as np
import torch


def init_random_seed(random_seed=0, rank=0):
    seed = random_seed + rank
    random.seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def init_dist_process(rank, temp_dir, num_gpus, random_seed, backend=None):
    """One process per GPU; RCCL ("nccl" backend on ROCm) over xGMI, file:// rendezvous as in the
    reference (utils.py:33-42).  `backend="gloo"` is used by the CPU tests."""
    init_random_seed(random_seed, rank)
    init_method = f"file://{(temp_dir / '.torch_distributed_init').resolve()}"
    backend = backend or ("nccl" if torch.cuda.is_available() else "gloo")
    torch.distributed.init_process_group(backend=backend, init_method=init_method, world_size=num_gpus, rank=rank)


def set_requires_grad(net, requires_grad: bool = True):
    for param in net.parameters():
        param.requires_grad = requires_grad


def sigmoid_to_tanh(x):
    """[0,1] -> [-1,+1]"""
    return x * 2.0 - 1.0


def tanh_to_sigmoid(x):
    """[-1,+1] -> [0,1]"""
    return (x + 1.0) / 2.0


def cycle(iterable):
    while True:
        yield from iterable


_LUTS = {}   # (colormap name, device) -> [256,3] fp32 on that device


def _named_lut(cmap, device):
    key = (cmap, torch.device(device))
    if key not in _LUTS:
        import matplotlib   # only a NAME needs it, and only the first time per device
        try:
            colormap = matplotlib.colormaps[cmap]
        except KeyError:
            raise ValueError(f"unknown cmap: {cmap}") from None
        colors = colormap(np.linspace(0, 1, 256))[:, :3]
        _LUTS[key] = torch.tensor(colors, device=device).float()
    return _LUTS[key]


def colorize(tensor, cmap="turbo"):
    """(B,1,H,W) or (B,H,W) in [0,1] -> (B,3,H,W) colours (reference: utils.py:167-191), one launch (dgv2_colorize).
    cmap: an ndarray [N,3], or the name of a matplotlib colormap (sampled at 256 points, cached per device)."""
    from gans.models.ops import native
    if tensor.ndim == 4:
        B, C, H, W = tensor.shape
        assert C == 1, f"expected (B,1,H,W) tensor, but got {tensor.shape}"
        tensor = tensor.squeeze(1)
    assert tensor.ndim == 3, f"got {tensor.ndim}!=3"
    if isinstance(cmap, np.ndarray):
        lut = torch.tensor(cmap, device=tensor.device).float()
    else:
        lut = _named_lut(cmap, tensor.device)
    return native.colorize_lut(tensor, lut)


def points_to_normal_2d(points_map, mode="closest", d=2):
    """(B,3,H,W) points -> normal colours in [0,1] (reference: utils.py:198-202)."""
    from gans.geometry import estimate_surface_normal
    normals = estimate_surface_normal(points_map, d=d, mode=mode).neg_()
    normals[normals != normals] = 0.0
    return tanh_to_sigmoid(normals).clamp_(0.0, 1.0)


def power_spectrum_2d(x):
    """(..., H, W) -> the centred 2-D power spectrum in dB (reference: utils.py:205-209).  A torch.fft composition: it
    runs once per image log."""
    spectrum = torch.fft.fftshift(torch.fft.fft2(x, norm="forward"), dim=[-1, -2])
    return 10 * torch.log10(spectrum.abs() ** 2)


class InfiniteSampler(torch.utils.data.Sampler):
    """Rank-sharded infinite shuffled index stream with a sliding re-shuffle window
    (reference: utils.py:238-271, from StyleGAN3)."""

    def __init__(self, dataset, rank=0, num_replicas=1, shuffle=True, seed=0, window_size=0.5):
        assert len(dataset) > 0 and num_replicas > 0 and 0 <= rank < num_replicas and 0 <= window_size <= 1
        self.dataset, self.rank, self.num_replicas = dataset, rank, num_replicas
        self.shuffle, self.seed, self.window_size = shuffle, seed, window_size

    def __iter__(self):
        order = np.arange(len(self.dataset))
        rnd, window = None, 0
        if self.shuffle:
            rnd = np.random.RandomState(self.seed)
            rnd.shuffle(order)
            window = int(np.rint(order.size * self.window_size))
        idx = 0
        while True:
            i = idx % order.size
            if idx % self.num_replicas == self.rank:
                yield order[i]
            if window >= 2:
                j = (i - rnd.randint(window)) % order.size
                order[i], order[j] = order[j], order[i]
            idx += 1
