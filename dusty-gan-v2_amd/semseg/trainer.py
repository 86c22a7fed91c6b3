"""Training of the range-image segmentation models, one process per GPU (reference: train_semseg.py:136-212 the
builders, 243-362 the loop).  The trunk's training forward and backward are the library composition under autograd (DESIGN.md
section 31); the loss is the native masked focal loss (section 29) and the tail of the step -- unscale, global-norm
clip, SGD with momentum, loss-scale update -- runs on csrc/sgd.hip (section 34), without a host synchronisation.

Several ranks (reference: train_semseg.py:172-174, 375-382): every BatchNorm2d becomes a semseg.models.SyncBatchNorm2d
(csrc/syncbn.hip, section 39) and the gradients are averaged over the ranks on one flat buffer
(gans.parallel.FlatGradSync) between the backward and the tail.  There is no DistributedDataParallel wrapper: the state
dict has no "module." prefix.

Not here: tensorboard images.
"""
import warnings

import torch
import torch.distributed as dist
import torch.nn.functional as F
from torch import optim

from gans import parallel
from gans.models.ops.native.sgd import fused_clip_sgd_step

from .config import to_plain
from .metrics import Evaluator
from .models import MaskedSegLoss, SqueezeSegV1, SqueezeSegV2, convert_sync_batchnorm

INIT_SCALE = 65536.0   # torch.amp.GradScaler's defaults
GROWTH, BACKOFF, GROWTH_INTERVAL = 2.0, 0.5, 2000


def build_model(cfg, pretrained_weights=True):
    """The model of cfg.arch for cfg.dataset.num_classes (train_semseg.py:136-170).  pretrained_weights goes to
    SqueezeSegV2 (its SqueezeNet initialisation); V2's classifier bias starts at the logit of cfg.dataset.logit_bias."""
    arch, crf = cfg.arch, cfg.arch.crf
    common = dict(inputs=list(arch.inputs), num_classes=cfg.dataset.num_classes, head_dropout_p=arch.decoder.dropout_p,
                  use_crf=arch.use_crf, crf_kernel_size=tuple(crf.kernel_size),
                  crf_init_weight_smoothness=crf.init_weight_smoothness,
                  crf_init_weight_appearance=crf.init_weight_appearance, crf_theta_gamma=crf.theta_gamma,
                  crf_theta_alpha=crf.theta_alpha, crf_theta_beta=crf.theta_beta, crf_num_iters=crf.num_iters)
    if arch.name == "squeezeseg_v1":
        return SqueezeSegV1(**common)
    if arch.name == "squeezeseg_v2":
        model = SqueezeSegV2(bn_momentum=arch.bn_momentum, pretrained_weights=pretrained_weights, **common)
        if cfg.dataset.get("logit_bias") is not None:
            prior = torch.tensor(cfg.dataset.logit_bias, dtype=torch.float32)
            model.decoder.head[1].bias.data = -torch.log((1 - prior) / prior)
        return model
    raise ValueError(arch.name)


def build_criterion(cfg):
    """MaskedSegLoss for cfg.loss (train_semseg.py:179-197): focal_loss with focal_gamma, or cross_entropy (gamma 0),
    either with the class weights cfg.loss.cls_weight."""
    alpha = torch.tensor(cfg.loss.cls_weight).float()
    if cfg.loss.name == "focal_loss":
        return MaskedSegLoss(gamma=float(cfg.loss.focal_gamma), alpha=alpha)
    if cfg.loss.name == "cross_entropy":
        return MaskedSegLoss(gamma=0.0, alpha=alpha)
    raise ValueError(cfg.loss.name)


def make_inputs(item, modalities):
    """The model's input image: the named modalities of the item stacked along the channels ([B,H,W] ones as one)."""
    return torch.cat([item[m] if item[m].ndim == 4 else item[m][:, None] for m in modalities], dim=1)


def resize_nearest(t, size):
    """A [B,H,W] label or mask map at another size (nearest-exact), dtype kept."""
    return F.interpolate(t[:, None].float(), size=size, mode="nearest-exact")[:, 0].to(t.dtype)


class Trainer:
    """Model, criterion, SGD, the exponential lr schedule and (cfg.use_amp) a device-resident loss scale.

    fused_optimizer=True: the step's tail is native.fused_clip_sgd_step.  False: torch's clip_grad_norm_ + SGD.step,
    with torch.amp.GradScaler under AMP -- the yardstick of section 34 and the fallback.  Both keep torch's optimizer
    state layout.  self.scale: float32 [2] (loss scale, growth tracker) on the device, None without AMP.
    self.conf_train: int64 [C+1,C+1] confusion counts of THIS rank's training predictions since the last reset_conf();
    conf_total() sums them over the ranks.

    Under a process group of several ranks (gans.parallel.is_dist()), or with sync_bn=True, the model's batch norms are
    the native synchronised ones; under a process group the parameters and buffers start as rank 0's and every step
    averages the gradients over the ranks before its tail, so a float16 overflow on one rank is non-finite on all of
    them and every rank skips and rescales alike.  One rank and sync_bn unset: nothing of this runs."""

    def __init__(self, cfg, device, fused_optimizer=True, pretrained_weights=True, sync_bn=None):
        self.cfg = cfg
        self.device = torch.device(device)
        self.fused_optimizer = bool(fused_optimizer)
        self.use_amp = bool(cfg.use_amp)
        self.num_classes = int(cfg.dataset.num_classes)
        self.model = build_model(cfg, pretrained_weights=pretrained_weights).to(self.device).train()
        self.distributed = parallel.is_dist()
        self.world_size = parallel.world_size()
        self.sync_bn = bool(sync_bn) or self.distributed
        if self.sync_bn:
            convert_sync_batchnorm(self.model)
        parallel.broadcast_module(self.model)
        self.grad_sync = parallel.FlatGradSync(self.model) if self.distributed else None
        self.criterion = build_criterion(cfg).to(self.device)
        tr = cfg.training
        self.optimizer = optim.SGD(list(self.model.parameters()), lr=tr.lr, momentum=tr.lr_momentum,
                                   weight_decay=tr.weight_decay)
        self.scheduler = optim.lr_scheduler.ExponentialLR(self.optimizer, gamma=tr.lr_decay)
        self.max_grad_norm = float(tr.max_grad_norm)
        self.loss_coef = float(cfg.loss.cls_loss_coef)
        self.scale = None
        self.grad_scaler = None
        if self.use_amp:
            self.scale = torch.tensor([INIT_SCALE, 0.0], device=self.device, dtype=torch.float32)
            if not self.fused_optimizer:
                self.grad_scaler = torch.amp.GradScaler("cuda", init_scale=INIT_SCALE, growth_factor=GROWTH,
                                                        backoff_factor=BACKOFF, growth_interval=GROWTH_INTERVAL)
        self.step_count = 0
        self.conf_train = torch.zeros((self.num_classes + 1, self.num_classes + 1), device=self.device, dtype=torch.int64)

    # ------------------------------------------------------------------------------------------------------------
    def _to_device(self, item):
        out = {k: v.to(self.device, non_blocking=True) for k, v in item.items()}
        out["label"] = out["label"].long()
        out["mask"] = out["mask"].float()
        return out

    def _forward(self, item):
        inputs = make_inputs(item, self.cfg.arch.inputs)
        with torch.autocast("cuda", dtype=torch.float16, enabled=self.use_amp):
            return self.model(inputs, item["xyz"], item["mask"])

    def reset_conf(self):
        self.conf_train.zero_()

    def conf_total(self):
        """conf_train summed over the ranks (a collective: every rank calls it at the same step); one rank: conf_train."""
        if not self.distributed:
            return self.conf_train
        total = self.conf_train.clone()
        dist.all_reduce(total, op=dist.ReduceOp.SUM)
        return total

    def _backward(self, loss):
        """Fresh gradients of `loss`; under a process group their average over the ranks, in the flat buffer."""
        if self.grad_sync is None:
            self.optimizer.zero_grad(set_to_none=True)
            loss.backward()
            return
        self.grad_sync.begin(direct=False)
        loss.backward()
        self.grad_sync.collect()
        self.grad_sync.all_reduce()

    def step(self, item):
        """One optimisation step on a batch {"xyz", "depth", "label", "mask"[, "reflectance"]} (any device).
        -> {"loss", "grad_norm", "pred"}: device tensors (the loss times cls_loss_coef, the unscaled total gradient
        norm before clipping, the masked predictions [B,H,W]).  No host synchronisation.  Afterwards p.grad still
        holds the raw gradient of loss * loss scale (fused path; torch's path leaves it unscaled and clipped)."""
        self.model.train()
        item = self._to_device(item)
        label, mask = item["label"], item["mask"]
        logit = self._forward(item)
        if isinstance(logit, tuple):   # deep supervision: one loss per scale, the scores from the last
            loss = 0
            for i, logit_i in enumerate(logit):
                size = tuple(logit_i.shape[-2:])
                last = i == len(logit) - 1
                loss_i, pred_i = self.criterion(logit_i, resize_nearest(label, size), resize_nearest(mask, size),
                                                conf=self.conf_train if last else None)
                loss = loss + loss_i
            pred = pred_i
        else:
            loss, pred = self.criterion(logit, label, mask, conf=self.conf_train)
        loss = loss * self.loss_coef

        if self.fused_optimizer:
            self._backward(loss * self.scale[0] if self.scale is not None else loss)
            sc = fused_clip_sgd_step(self.optimizer, self.max_grad_norm, scale_state=self.scale, growth=GROWTH,
                                     backoff=BACKOFF, growth_interval=GROWTH_INTERVAL)
            grad_norm = sc[0].clone()
        else:
            grad_norm = self._torch_tail(loss)
        self.step_count += 1
        if self.step_count % int(self.cfg.training.lr_decay_steps) == 0:
            with warnings.catch_warnings():
                # the fused tail never calls optimizer.step(), which is all the scheduler's order check looks at
                warnings.filterwarnings("ignore", message="Detected call of `lr_scheduler.step\\(\\)` before")
                self.scheduler.step()
        return {"loss": loss.detach(), "grad_norm": grad_norm, "pred": pred}

    def _torch_tail(self, loss):
        """The reference's lines 279-283 on torch's own kernels."""
        params = list(self.model.parameters())
        if self.grad_scaler is None:
            self._backward(loss)
            grad_norm = torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm)
            self.optimizer.step()
            return grad_norm.detach()
        self._backward(self.grad_scaler.scale(loss))
        self.grad_scaler.unscale_(self.optimizer)
        grad_norm = torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm)
        self.grad_scaler.step(self.optimizer)
        self.grad_scaler.update()
        return grad_norm.detach()

    def loss_scale(self):
        """The current loss scale as a Python float (reads back), None without AMP."""
        if not self.use_amp:
            return None
        if self.grad_scaler is not None:
            return float(self.grad_scaler.get_scale())
        return float(self.scale[0])

    # ------------------------------------------------------------------------------------------------------------
    def validate(self, loader, max_batches=None):
        """Scores of the model in eval() under inference_mode (the one-launch Fire path) over `loader`: the summary
        dict of semseg.metrics.Evaluator.  The model is left in train()."""
        evaluator = Evaluator(self.num_classes)
        self.model.eval()
        try:
            with torch.inference_mode():
                for i, item in enumerate(loader):
                    if max_batches is not None and i >= max_batches:
                        break
                    item = self._to_device(item)
                    logit = self._forward(item)
                    evaluator.update(logit[-1] if isinstance(logit, tuple) else logit, item["label"], item["mask"])
        finally:
            self.model.train()
        return evaluator.summary(mean_classes=slice(1, min(3, self.num_classes)))

    # ------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """The reference's checkpoint layout {"cfg", "step", "model", "optim"} (cfg as a plain dict) plus "scale"
        (loss scale, growth tracker; None without AMP).  The schedule is a function of "step" and is not stored."""
        if self.grad_scaler is not None:
            sd = self.grad_scaler.state_dict()
            scale = [float(sd["scale"]), float(sd["_growth_tracker"])]
        else:
            scale = None if self.scale is None else [float(v) for v in self.scale.tolist()]
        return {"cfg": to_plain(self.cfg), "step": self.step_count, "model": self.model.state_dict(),
                "optim": self.optimizer.state_dict(), "scale": scale}

    def load_state_dict(self, ckpt):
        """Adopts a checkpoint of state_dict()'s layout, or the reference's (no "scale": the loss scale restarts).
        The optimizer's lr in the checkpoint already carries the decays of its `step` steps."""
        self.model.load_state_dict(ckpt["model"])
        self.optimizer.load_state_dict(ckpt["optim"])
        self.step_count = int(ckpt["step"])
        decays = self.step_count // int(self.cfg.training.lr_decay_steps)
        self.scheduler.last_epoch = decays
        self.scheduler._last_lr = [g["lr"] for g in self.optimizer.param_groups]
        scale = ckpt.get("scale")
        if scale is not None and self.use_amp:
            self.scale.copy_(torch.tensor(scale, dtype=torch.float32))
            if self.grad_scaler is not None:
                self.grad_scaler.load_state_dict({"scale": float(scale[0]), "growth_factor": GROWTH, "backoff_factor": BACKOFF,
                                                  "growth_interval": GROWTH_INTERVAL, "_growth_tracker": int(scale[1])})


__all__ = ["Trainer", "build_model", "build_criterion", "make_inputs", "resize_nearest", "INIT_SCALE"]
