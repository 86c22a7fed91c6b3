"""Frontal range-image datasets of the SqueezeSeg line of work (reference: semseg/datasets/sqsg.py): the KITTI frontal
scans with per-point labels (KITTIRawFrontal), the GTA-LiDAR simulation with a ray-drop map sampled per item (GTALiDAR)
or with one GAN-made ray-drop map per scan (GTALiDAR_GAN), and SyntheticFrontal, a file-less stand-in with the same
item dict.  Constructors, item keys, dtypes, statistics and class lists are the reference's; its torchvision calls are
written out in torch (to_tensor: HWC -> CHW, resize(NEAREST): F.interpolate(mode="nearest"), normalize: (x - mean) / std).

One item, for a scan stored as [H, W, channels] with channels (x, y, z, [reflectance,] depth, label):
    mask = depth > 0 (times the ray-drop draw);  every channel but the label is multiplied by the mask, THEN normalised;
    a random flip mirrors the image and the mask along the width and negates the normalised y.
"""
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F


def _load_chw(path, shape):
    """A [H, W, C] .npy scan as a [C, shape[0], shape[1]] tensor, nearest-neighbour resized where the sizes differ."""
    points = torch.from_numpy(np.ascontiguousarray(np.load(path).transpose(2, 0, 1)))
    if tuple(points.shape[-2:]) != tuple(shape):
        points = F.interpolate(points[None], size=tuple(shape), mode="nearest")[0]
    return points


class _FrontalBase(torch.utils.data.Dataset):
    """What the file-backed datasets share.  A subclass defines MEAN / STD (one entry per stored channel, the label
    last with (0, 1)), DEPTH (the depth channel), CLASSES and SPLITS, implements load_datalist (fills self.datalist) and
    _path, and may override _raydrop."""

    def __init__(self, root, split, shape, min_depth, max_depth, flip):
        super().__init__()
        assert split in self.SPLITS, split
        self.root = Path(root)
        self.split = split
        self.shape = tuple(shape)
        self.min_depth = min_depth
        self.max_depth = max_depth
        self.flip = flip
        self.datalist = None
        self.load_datalist()

    def load_datalist(self):
        raise NotImplementedError

    def _path(self, index):
        raise NotImplementedError

    def _raydrop(self, index, mask):
        return mask

    def _item(self, index):
        """-> (points [C,H,W] masked and normalised, mask [H,W] float32), after the flip draw."""
        points = _load_chw(self._path(index), self.shape)
        mask = (points[self.DEPTH] > 0).float()
        mask = self._raydrop(index, mask)
        points[:-1] *= mask[None]
        points = (points - self.mean.to(points.dtype)[:, None, None]) / self.std.to(points.dtype)[:, None, None]
        draw = np.random.rand()   # drawn whether or not flipping is on, as the reference does
        if draw > 0.5 and self.flip:
            points = points.flip(-1)
            points[1] *= -1
            mask = mask.flip(-1)
        return points, mask

    @property
    def mean(self):
        return torch.tensor(self.MEAN)

    @property
    def std(self):
        return torch.tensor(self.STD)

    @property
    def class_list(self):
        return list(self.CLASSES)

    def __len__(self):
        return len(self.datalist)

    def _repr_lines(self):
        return [f"Number of datapoints: {len(self)}", f"Root location: {self.root}", f"Split: {self.split}"]

    def __repr__(self):
        return "\n".join(["Dataset " + type(self).__name__] + ["    " + line for line in self._repr_lines()])


class KITTIRawFrontal(_FrontalBase):
    """root/ImageSet/<split>.txt names the scans, root/lidar_2d/<name>.npy holds them: [H, W, 6] = (x, y, z,
    reflectance, depth, label).  omit_cyclist maps label 3 to 0 and drops the class from class_list."""

    MEAN = (10.88, 0.23, -1.04, 0.21, 12.12, 0.0)
    STD = (11.47, 6.91, 0.86, 0.16, 12.32, 1.0)
    DEPTH = 4
    CLASSES = ("unknown", "car", "pedestrian", "cyclist")
    SPLITS = ("all", "train", "val")

    def __init__(self, root="data/kitti_raw_frontal", split="train", shape=(64, 512), min_depth=1.45, max_depth=80.0,
                 flip=False, omit_cyclist=False):
        self.omit_cyclist = omit_cyclist
        super().__init__(root, split, shape, min_depth, max_depth, flip)

    def load_datalist(self):
        setlist = self.root / "ImageSet" / (self.split + ".txt")
        assert setlist.exists(), setlist
        with open(setlist) as f:
            self.datalist = [line.strip() + ".npy" for line in f]

    def _path(self, index):
        return self.root / "lidar_2d" / self.datalist[index]

    @property
    def class_list(self):
        return list(self.CLASSES[:3] if self.omit_cyclist else self.CLASSES)

    def __getitem__(self, index):
        points, mask = self._item(index)
        if self.omit_cyclist:
            points[5][points[5] == 3] = 0
        return {"xyz": points[:3].float(), "reflectance": points[[3]].float(), "depth": points[[4]].float(),
                "label": points[5].long(), "mask": mask}


class GTALiDAR(_FrontalBase):
    """root/GTAV/*/*.npy: [H, W, 5] = (x, y, z, depth, label).  raydrop_p: None, or a numpy map of keep probabilities
    of the dataset's shape; every item multiplies its mask by one Bernoulli draw of the map."""

    MEAN = (10.88, 0.23, -1.04, 12.12, 0.0)
    STD = (11.47, 6.91, 0.86, 12.32, 1.0)
    DEPTH = 3
    CLASSES = ("unknown", "car", "pedestrian")
    SPLITS = ("all",)

    def __init__(self, root="data/kitti_raw_frontal", split="all", shape=(64, 512), min_depth=1.45, max_depth=80.0,
                 flip=False, raydrop_p=None):
        super().__init__(root, split, shape, min_depth, max_depth, flip)
        if raydrop_p is None:
            self.dropout_map = torch.ones(self.shape)
        else:
            assert tuple(raydrop_p.shape) == self.shape
            self.dropout_map = torch.from_numpy(raydrop_p)

    def load_datalist(self):
        self.datalist = sorted((self.root / "GTAV").glob("*/*.npy"))

    def _path(self, index):
        return self.datalist[index]

    def _raydrop(self, index, mask):
        mask *= torch.bernoulli(self.dropout_map)
        return mask

    def __getitem__(self, index):
        points, mask = self._item(index)
        return {"xyz": points[:3].float(), "depth": points[[3]].float(), "label": points[4].long(), "mask": mask}


class GTALiDAR_GAN(GTALiDAR):
    """GTALiDAR whose ray-drop map is read per scan: the file of the same relative path under root/<gan_dir>/ (the
    maps a trained generator inferred for that scan)."""

    def __init__(self, root="data/kitti_raw_frontal", split="all", shape=(64, 512), min_depth=1.45, max_depth=80.0,
                 flip=False, gan_dir="GTAV_noise"):
        super().__init__(root, split, shape, min_depth, max_depth, flip, raydrop_p=None)
        self.gan_dir = gan_dir

    def _raydrop(self, index, mask):
        noise_path = str(self.datalist[index]).replace("GTAV", self.gan_dir)
        mask *= torch.bernoulli(torch.from_numpy(np.load(noise_path)).float())
        return mask

    def _repr_lines(self):
        return super()._repr_lines() + [f"GAN: {self.gan_dir}"]


_M64 = (1 << 64) - 1


def _hash_unit(seed, index, plane, n):
    """n reproducible values in [0, 1): a 64-bit integer mix (the splitmix64 finaliser) of (seed, index, plane,
    position), top 53 bits.  No random generator state is read or advanced."""
    with np.errstate(over="ignore"):
        key = (int(seed) * 0x9E3779B97F4A7C15 + int(index) * 0xBF58476D1CE4E5B9 + int(plane) * 0x94D049BB133111EB) & _M64
        z = np.arange(n, dtype=np.uint64) * np.uint64(0xD6E8FEB86659FD93) + np.uint64(key)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


class SyntheticFrontal(torch.utils.data.Dataset):
    """`length` deterministic frontal scans of `shape`, built in memory from an integer hash of (seed, index): a
    spherical grid (90 degrees of azimuth, +2 .. -24.8 degrees of elevation), depths between 2 and 60 m, about 15 % of
    the rays missing, labels in [0, num_classes) laid out in hashed blocks of 1 x 4 pixels.  The item dict, dtypes
    and normalisation are KITTIRawFrontal's.  Item i never depends on another item or on any global generator."""

    MEAN, STD = KITTIRawFrontal.MEAN, KITTIRawFrontal.STD

    def __init__(self, length=64, shape=(64, 512), num_classes=4, seed=0):
        super().__init__()
        self.length = int(length)
        self.shape = tuple(shape)
        self.num_classes = int(num_classes)
        self.seed = int(seed)
        H, W = self.shape
        elev = np.deg2rad(np.linspace(2.0, -24.8, H))[:, None]
        azim = np.deg2rad(np.linspace(45.0, -45.0, W))[None, :]
        self._dirs = np.stack([np.cos(elev) * np.cos(azim), np.cos(elev) * np.sin(azim), np.sin(elev) * np.ones_like(azim)])

    @property
    def class_list(self):
        return (list(KITTIRawFrontal.CLASSES) + [f"class_{c}" for c in range(4, self.num_classes)])[:self.num_classes]

    def __len__(self):
        return self.length

    def __getitem__(self, index):
        index = int(index)
        if not 0 <= index < self.length:
            raise IndexError(index)
        H, W = self.shape
        unit = lambda plane, n: _hash_unit(self.seed, index, plane, n)   # noqa: E731
        depth = 2.0 + 58.0 * unit(0, H * W).reshape(H, W) ** 2
        mask = (unit(1, H * W).reshape(H, W) < 0.85).astype(np.float32)
        blocks = (unit(2, H * ((W + 3) // 4)) * self.num_classes).astype(np.int64).reshape(H, -1)
        label = np.minimum(np.repeat(blocks, 4, axis=1)[:, :W], self.num_classes - 1)
        refl = unit(3, H * W).reshape(H, W)
        points = np.concatenate([self._dirs * depth[None], refl[None], depth[None]]).astype(np.float32)
        points = torch.from_numpy(points * mask[None])
        mean, std = torch.tensor(self.MEAN[:5]), torch.tensor(self.STD[:5])
        points = (points - mean[:, None, None]) / std[:, None, None]
        return {"xyz": points[:3], "reflectance": points[[3]], "depth": points[[4]], "label": torch.from_numpy(label),
                "mask": torch.from_numpy(mask)}


__all__ = ["KITTIRawFrontal", "GTALiDAR", "GTALiDAR_GAN", "SyntheticFrontal"]
