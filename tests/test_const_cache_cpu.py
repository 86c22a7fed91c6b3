"""CPU statement of the rule for caches of run constants (gans/models/ops/native/constcache.py): a hit
needs the same source objects at the same versions; a buffer a graph may have captured is refilled, never replaced;
nothing is kept with the switch off.  Needs the built library (the package imports dgv2_native), no GPU."""
import os
import re

import torch

from conftest import PKG
from gans.models.ops import FourierFeature
from gans.models.ops.native import constcache
from gans.models.ops.native.constcache import ConstCache, versioned


def _doubler(src, calls):
    def make():
        calls.append(1)
        return src * 2.0
    return make


def test_hit_calls_make_once():
    cache, src, calls = ConstCache(), torch.arange(6.0), []
    a = cache.get((src,), "k", _doubler(src, calls))
    b = cache.get((src,), "k", _doubler(src, calls))
    assert len(calls) == 1 and a is b and torch.equal(a, src * 2)
    cache.get((src,), "other", _doubler(src, calls))          # an unequal key misses
    assert len(calls) == 2


def test_modified_source_refills_in_place():
    cache, src, calls = ConstCache(), torch.arange(6.0), []
    a = cache.get((src,), None, _doubler(src, calls))
    ptr = a.data_ptr()
    src.add_(1)
    b = cache.get((src,), None, _doubler(src, calls))
    assert len(calls) == 2 and b is a and b.data_ptr() == ptr and torch.equal(b, (torch.arange(6.0) + 1) * 2)
    assert cache.get((src,), None, _doubler(src, calls)) is a and len(calls) == 2


def test_other_source_object_refills_in_place():
    cache, src, calls = ConstCache(), torch.arange(6.0), []
    a = cache.get((src,), None, _doubler(src, calls))
    ptr, twin = a.data_ptr(), src.clone()
    b = cache.get((twin,), None, _doubler(twin, calls))
    assert len(calls) == 2 and b is a and b.data_ptr() == ptr and torch.equal(b, src * 2)
    assert cache.entry[0][0] is twin            # the entry now holds the new source, so the old one misses again
    cache.get((src,), None, _doubler(src, calls))
    assert len(calls) == 3


def test_other_shape_is_a_new_allocation_and_the_old_tensor_is_not_written():
    cache, src, big, calls = ConstCache(), torch.arange(6.0), torch.arange(8.0), []
    a = cache.get((src,), None, _doubler(src, calls))
    b = cache.get((big,), None, _doubler(big, calls))
    assert b is not a and b.data_ptr() != a.data_ptr() and torch.equal(a, src * 2) and torch.equal(b, big * 2)
    other_dtype = cache.get((big,), "half", lambda: (big * 2).half())
    assert other_dtype is not b and torch.equal(b, big * 2)


def test_list_value_keeps_every_level_address():
    cache, src, calls = ConstCache(), torch.arange(16.0).reshape(4, 4), []

    def levels():
        calls.append(1)
        return [src[::4].clone(), src[::2].clone()]
    a = cache.get((src,), None, levels)
    ptrs = [t.data_ptr() for t in a]
    src.mul_(3)
    b = cache.get((src,), None, levels)
    assert len(calls) == 2 and b is a and [t.data_ptr() for t in b] == ptrs
    assert torch.equal(b[0], src[::4]) and torch.equal(b[1], src[::2])
    one = cache.get((src,), "shorter", lambda: [src[::4].clone()])       # another count: replaced, old levels unwritten
    assert one is not a and one[0].data_ptr() not in ptrs and torch.equal(a[0], src[::4])


def test_stale():
    cache, src, calls = ConstCache(), torch.arange(6.0), []
    assert cache.get((src,), None, _doubler(src, calls), stale=True) is None and cache.entry is None and not calls
    a = cache.get((src,), None, _doubler(src, calls))
    ptr, version = a.data_ptr(), src._version
    src.data.add_(5)             # (rewritten behind autograd's back, as a native call does: no version bump)
    assert src._version == version and cache.get((src,), None, _doubler(src, calls)) is a and len(calls) == 1
    b = cache.get((src,), None, _doubler(src, calls), stale=True)
    assert len(calls) == 2 and b is a and b.data_ptr() == ptr and torch.equal(b, (torch.arange(6.0) + 5) * 2)


def test_switch_off_keeps_nothing(monkeypatch):
    monkeypatch.setattr(constcache, "_CONST_CACHE", False)
    cache, src, calls = ConstCache(), torch.arange(6.0), []
    a = cache.get((src,), None, _doubler(src, calls))
    b = cache.get((src,), None, _doubler(src, calls))
    assert len(calls) == 2 and a is not b and cache.entry is None


def test_versioned():
    t, calls = torch.arange(6.0), []

    def make():
        calls.append(1)
        return t.double()
    a = versioned(t, "_memo", make)
    assert versioned(t, "_memo", make) is a and len(calls) == 1
    t.add_(1)
    b = versioned(t, "_memo", make)
    assert b is not a and len(calls) == 2 and torch.equal(b, t.double())
    assert versioned(t, "_memo", make, ok=lambda v: v.dtype == torch.float64) is b and len(calls) == 2
    c = versioned(t, "_memo", make, ok=lambda v: v.dtype == torch.float16)
    assert c is not b and len(calls) == 3 and versioned(t, "_memo", make) is c


def test_freqs_w_follows_load_state_dict():
    torch.manual_seed(0)
    pe = FourierFeature(resolution=(8, 32), num_freqs=64)
    fw = pe.freqs_w()
    assert fw.is_contiguous() and torch.equal(fw, pe.freqs.reshape(-1, 2)[:, 1]) and pe.freqs_w() is fw
    ptr = fw.data_ptr()
    sd = {k: v.clone() for k, v in pe.state_dict().items()}
    sd["freqs"] = sd["freqs"] * 1.5 + 0.25
    pe.load_state_dict(sd)
    fw2 = pe.freqs_w()
    assert fw2.data_ptr() == ptr and torch.equal(fw2, sd["freqs"].reshape(-1, 2)[:, 1])
    assert torch.equal(fw2, pe.freqs.reshape(-1, 2)[:, 1])


def test_the_rule_has_one_home():
    """No hand-written cache attribute is left outside constcache.py, and the switch is bound there alone."""
    written = re.compile(r"\._(enc|fw|pyr)(_src|_key)?\b|\._dgv2_(frag16|up_tables|up_gram|vals|vals_t)\b"
                         r"|[gs]etattr\([^)]*\"_((enc|fw|pyr)(_src|_key)?|dgv2_(frag16|up_tables|up_gram))\"")
    bound = re.compile(r"^\s*(_CONST_CACHE\s*=|from\s.*\bimport\b.*\b_CONST_CACHE\b)", re.M)
    files = []
    for top, _, names in os.walk(os.path.join(PKG, "gans")):
        files += [os.path.join(top, n) for n in names if n.endswith(".py")]
    assert len(files) > 40
    owners = []
    for path in files:
        with open(path) as f:
            text = f.read()
        if bound.search(text):
            owners.append(os.path.basename(path))
        if os.path.basename(path) != "constcache.py":
            assert not written.search(text), f"{path}: {written.search(text).group(0)}"
    assert owners == ["constcache.py"]
    for name in ("ops/fourier.py", "dusty_v2.py", "ops/native/modup.py"):
        with open(os.path.join(PKG, "gans", "models", *name.split("/"))) as f:
            text = f.read()
        assert "is_current_stream_capturing" not in text and "_refresh_in_place" not in text, name
