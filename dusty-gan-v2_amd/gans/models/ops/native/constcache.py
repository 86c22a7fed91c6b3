"""native.constcache: the one rule for caches of run constants (ConstCache), and the per-tensor memo (versioned).

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI; package docstring and DESIGN.md section 27: the import rules).
"""
import os

import torch

# DGV2_NO_CONST_CACHE=1 recomputes every run constant (PE table, operand image, angle pyramid, azimuth frequencies) per call
_CONST_CACHE = os.environ.get("DGV2_NO_CONST_CACHE") is None


class ConstCache:
    """One cached value (a tensor or a list of tensors) derived from source tensors that are constants of the run: the
    sensor's angle grid, the frequency / phase buffers, the PE table itself.  THE RULE:

    * A hit needs the very source OBJECTS of the entry (held by it, so their storage cannot be recycled into a false hit)
      at the `_version`s they had, and an equal key.  A fresh or modified source always misses.
    * A buffer a hipGraph may have captured is REFILLED, NEVER REPLACED: a miss that finds an entry of the same count,
      shapes, dtypes and device copies the fresh values into the entry's tensors and returns those.  A graph captured
      while the entry was live has its address baked in; an eager pass that replaced the tensor (after a load_state_dict
      bumped the buffers' versions, say) would free it under that graph -- round 6 met exactly this as NaNs from a
      captured D body beside an eager G body (tests/test_gpu_trainer.py, mode g_eager_d_graph).  Only an entry of
      another shape is replaced, and then the old tensors are not written.
    * Nothing is kept and no entry is touched while a hipGraph is being captured (a tensor born inside a capture belongs
      to that graph's memory pool), or with the switch off: make()'s result is returned as it is.
    """

    def __init__(self):
        self.entry = None                     # (sources, their versions, key, value)

    @staticmethod
    def on(owner, name):
        """The cache that rides on `owner` (a module, or the tensor a graph reads the value beside) under `name`."""
        if name not in owner.__dict__:
            setattr(owner, name, ConstCache())
        return owner.__dict__[name]

    def get(self, sources, key, make, stale=False):
        """The value of make() for `sources` (a tuple of tensors) and `key`, under the rule above.  stale: the sources were
        rewritten by a native call that bumps no version -- an existing entry is refilled where it lies, and without an
        entry nothing is made (None)."""
        ent, versions = self.entry, tuple(s._version for s in sources)
        if stale and ent is None:
            return None
        if (not stale and ent is not None and len(ent[0]) == len(sources) and all(a is b for a, b in zip(ent[0], sources))
                and ent[1] == versions and ent[2] == key):
            return ent[3]
        value = make()
        if not _CONST_CACHE or (any(s.is_cuda for s in sources) and torch.cuda.is_current_stream_capturing()):
            return value
        if ent is not None and type(ent[3]) is type(value):
            old, new = (ent[3], value) if isinstance(value, list) else ([ent[3]], [value])
            if len(old) == len(new) and all(a.shape == b.shape and a.dtype == b.dtype and a.device == b.device
                                            for a, b in zip(old, new)):
                for a, b in zip(old, new):
                    a.copy_(b)
                value = ent[3]
        self.entry = (tuple(sources), versions, key, value)
        return value


def versioned(t, name, make, ok=None):
    """A derived value (converted / transposed weights) stored ON tensor `t` as `name` = (t._version, value): returned
    while t is unmodified and ok(value) holds, else make() is stored and returned.  It does NOT follow ConstCache's capture
    rule: these memos ride on per-pass temporaries (`weight * gain`) born inside R1's capture and die with them;
    dropping them there would add conversions to the captured graph."""
    c = getattr(t, name, None)
    if c is not None and c[0] == t._version and (ok is None or ok(c[1])):
        return c[1]
    value = make()
    setattr(t, name, (t._version, value))
    return value


__all__ = ["ConstCache", "versioned"]
