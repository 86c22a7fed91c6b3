"""Checkpoints of the segmentation models (reference: semseg/pretrained.py, test_semseg.py:69-104).

    ckpt = load_checkpoint(path)                     # {"cfg", "step", "model", "optim"[, "scale"]}
    model = build_from_checkpoint(ckpt, "cuda:0")    # eval(), state dict loaded strict=True

Two kinds of file are read: what semseg.trainer.Trainer.state_dict() writes (cfg as plain dicts and lists) and the
reference's own layout, whose cfg is a pickled OmegaConf tree.  Both go through the restricted unpickler of
gans.pretrained: omegaconf is never imported, a file cannot name anything outside that module's allow-list, and nothing
is fetched from anywhere.  Whatever the file holds as cfg becomes plain containers and is merged over
semseg.config.default_config(), so a key the file lacks reads as the default."""
import os

import torch

from gans.config import to_config
from gans.pretrained import load_checkpoint as _load_restricted

from .config import default_config, merge, to_plain
from .trainer import build_model


def load_checkpoint(path, map_location="cpu"):
    """The checkpoint at `path` with ckpt["cfg"] a gans.config.Config carrying every key of default_config()."""
    path = os.fspath(path)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"semseg.pretrained.load_checkpoint: no file at {path} (nothing is downloaded)")
    ckpt = _load_restricted(path, map_location=map_location)
    if not isinstance(ckpt, dict) or "cfg" not in ckpt or "model" not in ckpt:
        raise ValueError(f"{path}: not a segmentation checkpoint (a dict with 'cfg' and 'model' is expected)")
    ckpt["cfg"] = to_config(merge(to_plain(default_config()), to_plain(ckpt["cfg"])))
    return ckpt


def build_from_checkpoint(ckpt, device):
    """The model of ckpt["cfg"] on `device`, in eval(), with ckpt["model"] loaded strict=True.  The SqueezeNet
    initialisation is skipped (pretrained_weights=False): the state dict overwrites every parameter."""
    model = build_model(ckpt["cfg"], pretrained_weights=False).to(device)
    model.load_state_dict(ckpt["model"], strict=True)
    return model.eval()


__all__ = ["load_checkpoint", "build_from_checkpoint"]
