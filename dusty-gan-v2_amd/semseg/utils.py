"""Helpers of the segmentation training loop (reference: semseg/utils.py)."""
import itertools

import numpy as np
import torch


class InfiniteSampler(torch.utils.data.Sampler):
    """The endless index stream of the reference's training loader (semseg/utils.py:238-271): the dataset is shuffled
    once; then the stream walks the permutation round and round, and after visiting a position it swaps that entry
    with the one a random distance (below window_size * len) behind it, so the order keeps drifting.  Replica `rank`
    of `num_replicas` is handed every num_replicas-th visit.

    The draws are the reference's -- one RandomState(seed).shuffle, then one randint(window) per visit, whichever
    replica the visit belongs to -- so equal arguments give equal indices.  shuffle=False walks 0 .. len-1 for ever."""

    def __init__(self, dataset, rank=0, num_replicas=1, shuffle=True, seed=0, window_size=0.5):
        if len(dataset) <= 0 or num_replicas <= 0 or not 0 <= rank < num_replicas or not 0 <= window_size <= 1:
            raise ValueError("InfiniteSampler: empty dataset, or rank / num_replicas / window_size out of range")
        super().__init__()
        self.dataset = dataset
        self.rank = rank
        self.num_replicas = num_replicas
        self.shuffle = shuffle
        self.seed = seed
        self.window_size = window_size

    def __iter__(self):
        n = len(self.dataset)
        perm = np.arange(n)
        rng, window = None, 0
        if self.shuffle:
            rng = np.random.RandomState(self.seed)
            rng.shuffle(perm)
            window = int(np.rint(n * self.window_size))
        for visit in itertools.count():
            here = visit % n
            if visit % self.num_replicas == self.rank:
                yield perm[here]
            if window >= 2:
                back = (here - rng.randint(window)) % n
                perm[here], perm[back] = perm[back], perm[here]


__all__ = ["InfiniteSampler"]
