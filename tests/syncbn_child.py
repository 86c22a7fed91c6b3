"""Child process of tests/test_gpu_syncbn.py: one rank of the data-parallel segmentation Trainer, or the one-process
run on the whole batch.  Writes what the parent compares to <out>/rank<r>.pt.

    python tests/syncbn_child.py <out_dir> <backend none|nccl|gloo> <world> <rank> <init_file>

The batch is the same four SyntheticFrontal scans in every run, mask all ones; rank r of `world` takes scans
[r * 4 / world, (r + 1) * 4 / world).  backend nccl: rank r on device r.  gloo: every rank on device 0 (RCCL refuses two
ranks on one device).  none: no process group, Trainer(sync_bn=True).  A one-rank nccl group runs under
DGV2_DIST_WORLD1 (set by the parent), so that gans.parallel treats it as distributed and every collective is issued.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dusty-gan-v2_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import torch
import torch.distributed as dist

SCANS, H, W = 4, 16, 64


def condition_trunk(model, seed=0):
    """A state the comparisons of tests/test_gpu_syncbn.py are meaningful on, drawn from `seed` alone.  Two things make
    the model's own start a comparison of noise with noise.  (1) Its encoder weights (standard deviation 0.001) leave
    activations whose variance is below the norms' eps: inverse deviations of 300 over thirty layers turn a rounding
    into a gradient error of 1e4.  Hence He-scaled weights and norm parameters away from (1, 0).  (2) A ReLU whose input
    is within a rounding of zero is open in one float32 implementation and shut in the next; at 2 x 5 x 16 x 64 the deep
    layers hold 128 values per channel, and one such unit moves their gradients by tenths.  With conv biases of 1 .. 2 the
    library's own float32 run disagreed with its float64 run on 2 of 1.2 million units, a double-internal norm on 4, and
    the gradients of the last encoder block moved by 25 %; on the GPU one unit behind a decoder's up-sampling conv did the
    same to everything in front of it, in one run of three.  Biases of 5 .. 6 on every conv and transposed conv that
    feeds a ReLU (the Fire modules', the stem's, the context-aggregation modules' squeeze) leave about one unit in a
    thousand shut and none near the kink; the norms that follow remove the offset."""
    from semseg.models.common import ConvReLUNorm, DeconvReLU
    from semseg.models.squeezeseg_v2 import CAM

    g = torch.Generator().manual_seed(seed)

    def fill(t, lo, hi):
        t.copy_((torch.rand(t.shape, generator=g) * (hi - lo) + lo).to(t))

    with torch.no_grad():
        for name, t in model.named_parameters():
            if t.ndim == 4 and "upsample" not in name:
                bound = (6.0 / (t.shape[1] * t.shape[2] * t.shape[3])) ** 0.5
                fill(t, -bound, bound)
        for m in model.modules():
            if isinstance(m, (ConvReLUNorm, DeconvReLU)):
                fill(m[0].bias, 5.0, 6.0)
            if isinstance(m, CAM):
                fill(m.attn[1].bias, 5.0, 6.0)
            if isinstance(m, torch.nn.BatchNorm2d):
                fill(m.running_mean, -0.2, 0.2)
                fill(m.running_var, 0.5, 1.5)
                fill(m.weight, 0.5, 1.5)
                fill(m.bias, -0.2, 0.2)
    return model


def child_cfg():
    from semseg.config import load_config

    cfg = load_config(os.path.join(ROOT, "tests", "golden", "semseg_cfg", "sim2real_w_gan_noise_dustyv2.yaml"))
    cfg.dataset.shape = [H, W]
    cfg.training.batch_size = SCANS
    cfg.training.lr_decay_steps = 10000
    cfg.use_amp = False
    cfg.arch.decoder.dropout_p = 0.0    # the head's channel dropout would draw per rank
    return cfg


def main():
    out_dir, backend, world, rank, init_file = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    device = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(device)
    if backend != "none":
        from gans import parallel
        parallel.init_process_group(backend, device=device, init_method=f"file://{init_file}", rank=rank, world_size=world)

    from semseg.datasets import SyntheticFrontal
    from semseg.models import SyncBatchNorm2d
    from semseg.trainer import Trainer

    torch.manual_seed(0)
    trainer = Trainer(child_cfg(), device, pretrained_weights=False, sync_bn=True)
    assert (trainer.grad_sync is not None) == (backend != "none")
    condition_trunk(trainer.model)       # the same draws on every rank
    ds = SyntheticFrontal(SCANS, (H, W), 3, seed=0)
    per = SCANS // world
    items = [ds[i] for i in range(rank * per, (rank + 1) * per)]
    item = {k: torch.stack([it[k] for it in items]) for k in items[0]}
    item["mask"] = torch.ones_like(item["mask"])

    first = trainer.model.encoder["conv_1b"][2]
    assert isinstance(first, SyncBatchNorm2d)
    # The library picks its conv algorithm by the batch size: the conv in front of this norm gave 2 + 2 scans other bits
    # than 4 scans (8 % of the elements, by up to 3.8e-6).  Scan by scan it cannot, so the norm sees the same input bits
    # in every run and what is compared is the norm.
    conv = trainer.model.encoder["conv_1b"][0]
    whole_forward = conv.forward
    conv.forward = lambda t: torch.cat([whole_forward(t[i:i + 1]) for i in range(t.shape[0])])
    seen = {}

    def hook(_module, _inputs, y):
        x, _weight, mean, invstd = y.grad_fn.saved_tensors
        seen.update(x=x.detach().clone(), y=y.detach().clone(), mean=mean.clone(), invstd=invstd.clone())

    handle = first.register_forward_hook(hook)
    out = trainer.step(item)
    handle.remove()
    torch.cuda.synchronize()
    state = {"params": [p.detach().cpu() for p in trainer.model.parameters()],
             "buffers": [b.detach().cpu() for b in trainer.model.buffers()],
             "loss": out["loss"].cpu(), "grad_norm": out["grad_norm"].cpu(), **{k: v.cpu() for k, v in seen.items()}}
    torch.save(state, os.path.join(out_dir, f"rank{rank}.pt"))
    if backend != "none":
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
