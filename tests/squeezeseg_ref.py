"""Shared by the SqueezeSeg fixture script and tests: the integer-hash fill that stands in for stored weights and
inputs, the fixture's case lists, and the evaluation-mode Fire forward restated in plain torch (transposed conv as
its tap rule, padding explicit).  No project code is imported here."""
import math

import numpy as np
import torch

# ---- hash fill ------------------------------------------------------------------------------------------------------
_MASK = np.uint64(0xFFFFFFFFFFFFFFFF)


def _fnv1a(text):
    h = 0xCBF29CE484222325
    for byte in text.encode():
        h = ((h ^ byte) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def hash_uniform(key, n):
    """n float64 values in [0, 1): splitmix64 of (FNV-1a of `key`) + flat index, top 53 bits; exact uint64 numpy."""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(_fnv1a(key))
        z = (z + np.uint64(0x9E3779B97F4A7C15)) & _MASK
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _MASK
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _MASK
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def hash_tensor(key, shape, lo, hi):
    """float32 tensor of `shape`, uniform in [lo, hi), from hash_uniform(key)."""
    n = int(np.prod(shape)) if len(shape) else 1
    v = lo + (hi - lo) * hash_uniform(key, n)
    return torch.from_numpy(v.astype(np.float32).reshape(tuple(shape)))


def hash_fill_state_dict(sd, salt=""):
    """A new state dict with every tensor of `sd` replaced by hashed values of its key (CRF entries are kept):
    conv weights uniform with He's variance 2 / fan_in (a transposed (1,4) stride-2 conv has two taps per output),
    biases and running means in [-0.3, 0.3), batch-norm weights and running variances in [0.5, 1.5)."""
    out = {}
    for key, t in sd.items():
        if key.startswith("crf.") or key.endswith("num_batches_tracked"):
            out[key] = t.clone()
            continue
        name = salt + key
        if t.ndim == 4:
            if ".upsample." in key or key.startswith("upsample."):
                fan_in = t.shape[0] * 2
            else:
                fan_in = t.shape[1] * t.shape[2] * t.shape[3]
            a = math.sqrt(3.0 * 2.0 / fan_in)
            out[key] = hash_tensor(name, t.shape, -a, a)
        elif key.endswith("running_var") or (key.endswith(".weight") and t.ndim == 1):
            out[key] = hash_tensor(name, t.shape, 0.5, 1.5)
        else:
            out[key] = hash_tensor(name, t.shape, -0.3, 0.3)
    return out


# ---- the fixture's cases --------------------------------------------------------------------------------------------
# (version, B, Cin, Cs, E, H, W, up)
FIRE_CASES = [
    (2, 1, 16, 16, 16, 1, 1, False),      # smallest shape
    (2, 1, 16, 16, 16, 1, 1, True),       # smallest shape with up-sampling
    (2, 2, 64, 16, 64, 3, 33, False),     # ragged width
    (2, 1, 128, 32, 32, 9, 70, True),     # several tiles on both axes, ragged, up
    (2, 1, 384, 48, 192, 5, 17, False),   # Cs = 48
    (2, 1, 512, 64, 256, 2, 5, False),    # widest channels
    (1, 2, 64, 16, 64, 3, 33, False),     # V1 twins of the third and fourth
    (1, 1, 128, 32, 32, 9, 70, True),
]
# (version, B, H, W, use_crf); five input channels, four classes
MODEL_CASES = [(1, 1, 2, 16, False), (1, 2, 3, 48, False), (2, 1, 2, 16, False), (2, 2, 3, 48, False), (2, 1, 2, 16, True)]
MODEL_INPUTS, MODEL_CLASSES = ["xyz", "depth", "mask"], 4
SAMPLE_MAX = 4096   # outputs larger than this are stored at a hashed sample of their flat indices


def fire_case_name(i):
    v, B, Cin, Cs, E, H, W, up = FIRE_CASES[i]
    return f"fire{i}_v{v}_{B}x{Cin}x{H}x{W}_s{Cs}_e{E}{'_up' if up else ''}"


def model_case_name(i):
    v, B, H, W, crf = MODEL_CASES[i]
    return f"model{i}_v{v}_{B}x{H}x{W}{'_crf' if crf else ''}"


def fire_case_input(i):
    v, B, Cin, Cs, E, H, W, up = FIRE_CASES[i]
    return hash_tensor(fire_case_name(i) + "/x", (B, Cin, H, W), -1.5, 1.5)


def sample_index(name, numel):
    """The flat output indices a fixture stores: all of them up to SAMPLE_MAX, else SAMPLE_MAX hashed ones (sorted,
    possibly repeated)."""
    if numel <= SAMPLE_MAX:
        return torch.arange(numel)
    idx = np.sort((hash_uniform(name + "/sample", SAMPLE_MAX) * numel).astype(np.int64))
    return torch.from_numpy(idx)


def model_case_inputs(i):
    """img [B,5,H,W] (xyz, depth, mask), xyz [B,3,H,W] in metres-like range, mask [B,1,H,W] of 0 / 1."""
    v, B, H, W, crf = MODEL_CASES[i]
    name = model_case_name(i)
    xyz = hash_tensor(name + "/xyz", (B, 3, H, W), -1.0, 1.0)
    depth = hash_tensor(name + "/depth", (B, 1, H, W), 0.0, 1.0)
    mask = (hash_tensor(name + "/mask", (B, 1, H, W), 0.0, 1.0) < 0.85).float()
    return torch.cat([xyz, depth, mask], dim=1), xyz, mask


def listing(sd):
    """State-dict listing as one string per entry: key|shape|dtype."""
    return [f"{k}|{'x'.join(str(d) for d in v.shape)}|{str(v.dtype).replace('torch.', '')}" for k, v in sd.items()]


# ---- the Fire forward, restated -------------------------------------------------------------------------------------
def _affine(v, sd, prefix, eps):
    """Evaluation batch norm of the Sequential at `prefix` (index 2), or the identity where it has none."""
    if prefix + ".2.running_mean" not in sd:
        return v
    mean, var = sd[prefix + ".2.running_mean"], sd[prefix + ".2.running_var"]
    gamma, beta = sd[prefix + ".2.weight"], sd[prefix + ".2.bias"]
    shape = (1, -1, 1, 1)
    return (v - mean.view(shape)) * (gamma / torch.sqrt(var + eps)).view(shape) + beta.view(shape)


def fire_ref(sd, x, skip=None, eps=1e-5, dtype=torch.float64):
    """The evaluation-mode Fire module of state dict `sd` (V1 or V2 layout, with or without `upsample`) on x
    [B,Cin,H,W], everything cast to `dtype`.  einsum and shifted slices only."""
    sd = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    x = x.to(dtype)
    B, _, H, W = x.shape
    s = torch.einsum("oc,bchw->bohw", sd["squeeze1x1.0.weight"][:, :, 0, 0], x) + sd["squeeze1x1.0.bias"].view(1, -1, 1, 1)
    s = _affine(torch.relu(s), sd, "squeeze1x1", eps)
    if "upsample.0.weight" in sd:
        wd = sd["upsample.0.weight"]                      # [in, out, 1, 4]
        u = torch.zeros(B, wd.shape[1], H, 2 * W, dtype=dtype)
        for w in range(W):
            for k in range(4):
                wo = 2 * w - 1 + k
                if 0 <= wo < 2 * W:
                    u[:, :, :, wo] += torch.einsum("io,bih->boh", wd[:, :, 0, k], s[:, :, :, w])
        u = torch.relu(u + sd["upsample.0.bias"].view(1, -1, 1, 1))
    else:
        u = s
    Wo = u.shape[3]
    e1 = torch.einsum("oc,bchw->bohw", sd["expand1x1.0.weight"][:, :, 0, 0], u) + sd["expand1x1.0.bias"].view(1, -1, 1, 1)
    e1 = _affine(torch.relu(e1), sd, "expand1x1", eps)
    w3 = sd["expand3x3.0.weight"]
    up = torch.zeros(B, u.shape[1], H + 2, Wo + 2, dtype=dtype)   # u with its zero border: the padding is of u
    up[:, :, 1:H + 1, 1:Wo + 1] = u
    e3 = torch.zeros(B, w3.shape[0], H, Wo, dtype=dtype)
    for dy in range(3):
        for dx in range(3):
            e3 += torch.einsum("oc,bchw->bohw", w3[:, :, dy, dx], up[:, :, dy:dy + H, dx:dx + Wo])
    e3 = _affine(torch.relu(e3 + sd["expand3x3.0.bias"].view(1, -1, 1, 1)), sd, "expand3x3", eps)
    y = torch.cat([e1, e3], dim=1)
    return y if skip is None else y + skip.to(dtype)
