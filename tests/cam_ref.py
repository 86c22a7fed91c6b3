"""Shared by the context-aggregation fixture script and its tests: the fixture's case list, the hashed inputs and
weights (the integer hash of squeezeseg_ref) and the evaluation-mode module restated in plain torch -- the 7x7
maximum as 49 shifted slices of an explicitly -inf-padded tensor, the two 1x1 convs as einsums.  No project code is
imported here."""
import torch

from squeezeseg_ref import hash_fill_state_dict, hash_tensor, sample_index  # noqa: F401  (re-exported for the tests)

RADIUS = 3
# (B, C, H, W, kind): kind "plain" draws x in [-1.5, 1.5); "negative" in [-5, -1): every value is below the 0 a wrong
# padding would insert; "corners" puts every channel's maximum on one of the four image corners
CAM_CASES = [
    (1, 16, 1, 1, "plain"),        # the window is all padding but one pixel; Cr = 1
    (2, 64, 3, 33, "plain"),       # H < 7, a width off every tile multiple, two samples
    (1, 128, 9, 70, "plain"),      # widest channels, several tiles on both axes, ragged
    (1, 64, 8, 40, "negative"),    # all-negative input: zero padding is wrong in every border pixel
    (1, 32, 10, 45, "corners"),    # the maxima sit where a clipped or shifted window loses them
]
REDUCTION = 16


def cam_case_name(i):
    B, C, H, W, kind = CAM_CASES[i]
    return f"cam{i}_{B}x{C}x{H}x{W}_{kind}"


def cam_case_input(i):
    B, C, H, W, kind = CAM_CASES[i]
    name = cam_case_name(i)
    if kind == "negative":
        return hash_tensor(name + "/x", (B, C, H, W), -5.0, -1.0)
    x = hash_tensor(name + "/x", (B, C, H, W), -1.5, 1.5)
    if kind == "corners":
        peak = hash_tensor(name + "/peak", (B, C), 2.0, 3.0)
        for c in range(C):
            h, w = ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))[c % 4]
            x[:, c, h, w] = peak[:, c]
    return x


def cam_case_state_dict(i, template):
    """Hashed values for the state dict `template` of a context-aggregation module of case i's width."""
    return hash_fill_state_dict(template, salt=cam_case_name(i) + "/")


def border_mask(H, W):
    """bool [H,W]: the pixels whose 7x7 window leaves the image."""
    m = torch.zeros(H, W, dtype=torch.bool)
    m[:RADIUS], m[-RADIUS:], m[:, :RADIUS], m[:, -RADIUS:] = True, True, True, True
    return m


def cam_ref(sd, x, dtype=torch.float64):
    """The evaluation-mode module of state dict `sd` (attn.1 / attn.3: the squeeze and excite convs) on x [B,C,H,W],
    everything cast to `dtype`."""
    w1, b1 = sd["attn.1.weight"].to(dtype)[:, :, 0, 0], sd["attn.1.bias"].to(dtype)
    w2, b2 = sd["attn.3.weight"].to(dtype)[:, :, 0, 0], sd["attn.3.bias"].to(dtype)
    x = x.to(dtype)
    B, C, H, W = x.shape
    R = RADIUS
    padded = torch.full((B, C, H + 2 * R, W + 2 * R), float("-inf"), dtype=dtype)
    padded[:, :, R:R + H, R:R + W] = x
    m = padded[:, :, R:R + H, R:R + W].clone()
    for dy in range(2 * R + 1):
        for dx in range(2 * R + 1):
            m = torch.maximum(m, padded[:, :, dy:dy + H, dx:dx + W])
    a = torch.relu(torch.einsum("jc,bchw->bjhw", w1, m) + b1.view(1, -1, 1, 1))
    s = torch.einsum("cj,bjhw->bchw", w2, a) + b2.view(1, -1, 1, 1)
    return x * (1.0 / (1.0 + torch.exp(-s)))
