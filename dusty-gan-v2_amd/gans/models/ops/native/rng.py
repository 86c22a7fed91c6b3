"""native.rng: the Philox stream of a device and every random number of a step body from one launch.

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI; package docstring and DESIGN.md section 27: the import rules).
"""
import ctypes as _ct
import math

import torch

import dgv2_native as N


# ---------------------------------------------------------------------------------------
# every random number of a step body from one launch (dgv2_rng_fill, csrc/rng.hip)
# ---------------------------------------------------------------------------------------
_RNG_STATE = {}
RNG_UNIFORM, RNG_NORMAL, RNG_CLAMPED, RNG_BERNOULLI = 0, 1, 2, 3


def rng_state(device=None, seed=None):
    """The Philox stream of `device` (int64[4] device tensor: seed, offset, ticket, unused), created on first use from
    torch's seed of that moment (torch.initial_seed(): init_random_seed / manual_seed decide it, per rank).  `seed`
    re-seeds the stream and rewinds it.  Must exist before a hipGraph capture that draws from it."""
    idx = torch.cuda.current_device() if device is None else torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    st = _RNG_STATE.get(idx)
    if st is None or seed is not None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("dgv2: the RNG stream must exist before a hipGraph capture (native.rng_state())")
        sd = torch.initial_seed() if seed is None else int(seed)
        vals = torch.tensor([sd & 0x7FFFFFFFFFFFFFFF, 0, 0, 0], dtype=torch.int64)
        if st is None:
            st = _RNG_STATE[idx] = vals.to(torch.device("cuda", idx))
        else:
            st.copy_(vals)
    return st


def rng_fill(specs, device):
    """specs: list of (shape, kind, a, b) -> list of fp32 tensors (views of one allocation), ONE launch.
    kind RNG_UNIFORM: uniform in [a, b); RNG_NORMAL: mean a, std b; RNG_CLAMPED: u in [0, 1) clamped to [a, b];
    RNG_BERNOULLI: 1.0 with probability a, else 0.0."""
    if not 1 <= len(specs) <= 16:
        raise ValueError("rng_fill takes 1..16 segments")
    counts = [int(math.prod(sh)) for sh, _, _, _ in specs]
    offs, tot = [], 0
    for c in counts:
        offs.append(tot)
        tot += (c + 3) // 4 * 4            # 16-byte aligned segments: whole float4 stores
    st = rng_state(device)
    buf = torch.empty(tot, device=device, dtype=torch.float32)
    outs = [buf[o:o + c].view(sh) for o, c, (sh, _, _, _) in zip(offs, counts, specs)]
    n = len(specs)
    ptrs = N.ptr_array(outs)
    cnt = (_ct.c_int64 * n)(*counts)
    kinds = N.int_array([k for _, k, _, _ in specs])
    a = (_ct.c_float * n)(*[float(v) for _, _, v, _ in specs])
    b = (_ct.c_float * n)(*[float(v) for _, _, _, v in specs])
    N.call("dgv2_rng_fill", ptrs, cnt, kinds, a, b, n, N.ptr(st), N.stream())
    return outs


__all__ = ["RNG_UNIFORM", "RNG_NORMAL", "RNG_CLAMPED", "RNG_BERNOULLI", "rng_state", "rng_fill"]
