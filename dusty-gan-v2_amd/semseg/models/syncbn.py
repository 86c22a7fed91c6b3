"""Batch norm of the segmentation trunks whose training statistics run over every rank's samples (reference:
train_semseg.py:172-174, SyncBatchNorm.convert_sync_batchnorm), on gans.models.ops.native.syncbn.
"""
from torch import nn

from gans.models.ops.native import syncbn as _syncbn


class SyncBatchNorm2d(nn.BatchNorm2d):
    """nn.BatchNorm2d with the same parameters and buffers under the same names.  eval(), or a tensor that is not on a
    GPU: nn.BatchNorm2d.forward itself.  train() on a GPU tensor: native.sync_batch_norm over `group` (None: the default
    process group; without one, or with one rank, this process's batch -- the same kernels, no collective)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, group=None, **kw):
        super().__init__(num_features, eps, momentum, affine, track_running_stats, **kw)
        self.group = group

    def forward(self, x):
        if not (x.is_cuda and (self.training or not self.track_running_stats)):
            return super().forward(x)
        self._check_input_dim(x)
        keep = self.training and self.track_running_stats
        return _syncbn.sync_batch_norm(x, self.weight, self.bias, self.running_mean if keep else None,
                                       self.running_var if keep else None, self.num_batches_tracked if keep else None,
                                       self.eps, self.momentum, group=self.group)


def convert_sync_batchnorm(model, group=None):
    """Swaps every nn.BatchNorm2d of `model` for a SyncBatchNorm2d IN PLACE and returns the model; the new modules hold
    the old ones' tensors, so state dicts, optimizers and references to the parameters stay valid."""
    if type(model) is nn.BatchNorm2d:
        return _converted(model, group)
    for name, child in model.named_children():
        if type(child) is nn.BatchNorm2d:
            setattr(model, name, _converted(child, group))
        else:
            convert_sync_batchnorm(child, group)
    return model


def _converted(bn, group):
    new = SyncBatchNorm2d(bn.num_features, bn.eps, bn.momentum, bn.affine, bn.track_running_stats, group=group)
    if bn.affine:
        new.weight, new.bias = bn.weight, bn.bias
    for name in ("running_mean", "running_var", "num_batches_tracked"):
        new._buffers[name] = bn._buffers[name]
    new.training = bn.training
    return new


__all__ = ["SyncBatchNorm2d", "convert_sync_batchnorm"]
