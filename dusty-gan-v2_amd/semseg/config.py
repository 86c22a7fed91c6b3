"""Configuration of the segmentation trainer: the keys of the reference's configs/semseg/*.yaml as a Python dict
(default_config: the values its real2real.yaml carries) and load_config, which merges a YAML file over it.  The nodes
are gans.config.Config (nested dicts with attribute access)."""
import copy

import yaml

from gans.config import to_config

_DEFAULT = {
    "arch": {
        "name": "squeezeseg_v2",
        "inputs": ["xyz", "depth"],
        "bn_momentum": 0.001,
        "encoder": {"dropout_p": 0.5},
        "decoder": {"dropout_p": 0.5},
        "use_crf": True,
        "crf": {
            "kernel_size": [3, 5],
            "init_weight_smoothness": 0.02,
            "init_weight_appearance": 0.1,
            "theta_gamma": [0.9, 0.9, 0.6, 0.6],
            "theta_alpha": [0.9, 0.9, 0.6, 0.6],
            "theta_beta": [0.015, 0.015, 0.01, 0.01],
            "num_iters": 3,
        },
    },
    "dataset": {
        "name": "kitti_raw_frontal",
        "num_classes": 4,
        "logit_bias": [0.01, 0.33, 0.33, 0.33],
        "scan_unfolding": True,
        "shape": [64, 512],
        "random_flip": True,
    },
    "loss": {
        "name": "focal_loss",
        "focal_gamma": 2,
        "cls_loss_coef": 15.0,
        "cls_weight": [0.33, 1.0, 3.5, 3.5],
    },
    "training": {
        "max_steps": 50000,
        "lr": 0.05,
        "lr_momentum": 0.9,
        "lr_decay": 0.5,
        "lr_decay_steps": 10000,
        "weight_decay": 0.0001,
        "max_grad_norm": 1.0,
        "batch_size": 40,
        "checkpoint": {"test": 1000, "stats": 500, "image": 500},
    },
    "random_seed": 0,
    "channels_last": False,
    "use_amp": True,
}


def default_config():
    """A fresh Config with every key the trainer reads."""
    return to_config(copy.deepcopy(_DEFAULT))


def merge(base, over):
    """`over` laid over `base`, dict by dict; lists and scalars of `over` replace those of `base`.  Returns `base`."""
    for key, val in over.items():
        if isinstance(val, dict) and isinstance(base.get(key), dict):
            merge(base[key], val)
        else:
            base[key] = val
    return base


def load_config(path):
    """default_config() with the YAML file at `path` merged over it."""
    with open(path) as f:
        over = yaml.safe_load(f) or {}
    return to_config(merge(copy.deepcopy(_DEFAULT), over))


def to_plain(cfg):
    """A Config as plain dicts / lists / scalars (what a checkpoint stores)."""
    if isinstance(cfg, dict):
        return {k: to_plain(v) for k, v in cfg.items()}
    if isinstance(cfg, (list, tuple)):
        return [to_plain(v) for v in cfg]
    return cfg


__all__ = ["default_config", "load_config", "merge", "to_plain"]
