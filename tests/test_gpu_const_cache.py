"""The rule for caches of run constants (gans/models/ops/native/constcache.py) on the device: an address
a hipGraph captured survives a refresh of the PE table and of its operand image; nothing is kept from inside a capture;
a miss inside a capture leaves an entry alone.  256 pixels x 64 channels: the smallest table pe_frag16 takes (its pixel
count a multiple of 16, its channels of 32)."""
import pytest
import torch

from gans.models.ops import FourierFeature, native
from gans.models.ops.native.constcache import ConstCache

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pe(seed):
    torch.manual_seed(seed)
    return FourierFeature(resolution=(8, 32), num_freqs=64).to(DEV)


def _capture(body):
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        body()
    return graph


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_captured_addresses_survive_a_refresh(dtype):
    pe = _pe(0)
    angle = ((torch.rand(1, 2, 8, 32, generator=torch.Generator().manual_seed(1)) * 2 - 1) * 3.0).to(DEV)
    table = pe.encoded(angle, dtype)
    image = native.pe_frag16(table) if dtype == torch.bfloat16 else None      # (the operand image is a bf16 matter)
    assert tuple(table.shape) == (1, 8, 32, 64) and table.dtype == dtype
    before = table.clone()
    out_t, out_i = torch.zeros_like(table), None if image is None else torch.zeros_like(image)

    def body():
        out_t.copy_(table)
        if image is not None:
            out_i.copy_(image)
    graph = _capture(body)

    donor = _pe(7)                                                # other frequencies and phases, written in place
    pe.load_state_dict(donor.state_dict())
    again = pe.encoded(angle, dtype)
    # FIRST the addresses: an implementation that replaced a tensor fails here and never replays on a freed address
    assert again is table and again.data_ptr() == table.data_ptr()
    if image is not None:
        assert native.pe_frag16(again) is image
    graph.replay()
    torch.cuda.synchronize()

    fresh = _pe(3)
    fresh.load_state_dict(pe.state_dict())
    want_t = fresh.encoded(angle.clone(), dtype)
    assert want_t.data_ptr() != table.data_ptr() and not torch.equal(want_t, before)     # the refresh changed the table
    assert torch.equal(out_t, want_t)
    if image is not None:
        assert torch.equal(out_i, native.pe_frag16(want_t))


def test_nothing_is_kept_from_inside_a_capture():
    cache, src, calls = ConstCache(), torch.arange(64.0, device=DEV), []

    def make():
        calls.append(1)
        return src * 2.0
    got = []
    graph = _capture(lambda: got.append(cache.get((src,), None, make)))
    assert len(calls) == 1 and cache.entry is None
    eager = cache.get((src,), None, make)
    assert len(calls) == 2 and cache.entry is not None and eager is not got[0]
    assert torch.equal(eager, src * 2.0)
    del graph


def test_a_miss_inside_a_capture_leaves_the_entry_alone():
    cache, src, calls = ConstCache(), torch.arange(64.0, device=DEV), []

    def make():
        calls.append(1)
        return src * 2.0
    held = cache.get((src,), None, make)
    entry, ptr, values = cache.entry, held.data_ptr(), held.clone()
    src.add_(1)                                                   # the entry is out of date: the next lookup misses
    got = []
    graph = _capture(lambda: got.append(cache.get((src,), None, make)))
    graph.replay()
    torch.cuda.synchronize()
    assert len(calls) == 2 and got[0] is not held and torch.equal(got[0], src * 2.0)
    assert cache.entry is entry and cache.entry[3] is held and held.data_ptr() == ptr and torch.equal(held, values)
    assert cache.get((src,), None, make) is held and len(calls) == 3 and torch.equal(held, src * 2.0)   # eager: refilled
