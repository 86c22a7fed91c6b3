"""native.modgemm: batched channel GEMM of the modulated 1x1 conv -- engine routing, raw NN / TN calls, three autograd nodes.

Part of gans.models.ops.native (wrappers around the libdgv2 C ABI; package docstring and DESIGN.md section 27: the import rules).
"""
import math
import os

import torch
from torch.autograd import Function

import dgv2_native as N
from .act_resample import _BiasActBackward, _dt, _sq_tail
from .constcache import versioned


# ---------------------------------------------------------------------------------------
# batched channel GEMM = contraction of the modulated 1x1 conv
# (reference: grouped F.conv2d in ModConv2d.forward, gans/models/ops/style.py:105-118)
# ---------------------------------------------------------------------------------------
_HEAD_FWD = os.environ.get("DGV2_NO_HEAD_FWD") is None   # A/B switch for benchmarking
_PE_FWD = os.environ.get("DGV2_NO_PE_FWD") is None               # A/B switch for benchmarking
# (I, O) -> smallest pixel count from which the sample-walking kernel (dgv2_modconv_pe_fwd_sq, PE-free form) takes a
# per-sample-weight contraction.  Measured at B = 64 (scripts/mb_midgemm.py, profiles/round5_mb_midgemm.txt): it runs these
# shapes 3.4-3.9x faster than the generic NN engine (whose 128 x 128 tiles re-stage 32-128 KB of per-sample weights per
# block for four K-steps of work); round 5 added the 128- and 256-channel shapes of levels 2 / 1.
_PE_FREE_MINP = {(64, 32): 4096, (32, 64): 4096, (32, 32): 4096, (64, 64): 4096, (128, 64): 2048, (64, 128): 2048,
                 (128, 128): 1024, (256, 256): 512, (256, 128): 512, (128, 256): 512}
if os.environ.get("DGV2_NO_PE_MID"):   # A/B switch: the round-4 routing
    _PE_FREE_MINP = {k: 4096 for k in ((64, 32), (32, 64), (128, 64), (64, 128), (32, 32), (64, 64))}


# A/B switch: the bf16 per-sample-weight contractions of the generator's two lowest levels on gemm_stream.hip (stages of
# four K-steps, deeper loads in flight; the same bits as the generic engines).  A module flag read at call
# time, so that both paths can run in one process.
_GEMM_STREAM = os.environ.get("DGV2_NO_GEMM_STREAM") is None
# The routing is held to the geometries the kernel table was measured at (scripts/mb_gemm_lowlevels.py: the generator's
# 4 x 32 and 8 x 64 levels, per-sample weights): maps of at most 512 pixels.  The entries themselves take more (many pixel
# tiles, batch-shared weights: tests/test_gpu_gemm_stream.py), but nothing has shown that those shapes gain.
_GEMM_STREAM_MAX_P = 512


def _stream_wanted(P, per_sample=True):
    return _GEMM_STREAM and per_sample and P <= _GEMM_STREAM_MAX_P


def bmm_nn_sq_call(*args, per_sample=None):
    """dgv2_bmm_nn_sq(*args), on dgv2_gemm_stream_nn where the switch is on and the entry covers the geometry.
    per_sample: whether the weights count as per-sample for that routing; None: they do unless the batch shares one
    (wstride == 0)."""
    per_sample = args[9] != 0 if per_sample is None else per_sample   # wstride
    if not (_stream_wanted(args[4], per_sample) and N.try_call("dgv2_gemm_stream_nn", *args)):   # P
        N.call("dgv2_bmm_nn_sq", *args)


def bmm_nn_cat_sq_call(*args):
    """dgv2_bmm_nn_cat_sq(*args), on dgv2_gemm_stream_nn_cat where the switch is on and the entry covers the geometry."""
    if not (_stream_wanted(args[5]) and N.try_call("dgv2_gemm_stream_nn_cat", *args)):
        N.call("dgv2_bmm_nn_cat_sq", *args)


def bmm_tn_call(*args):
    """dgv2_bmm_tn(*args), on dgv2_gemm_stream_tn where the switch is on and the entry covers the geometry."""
    if not (_stream_wanted(args[4]) and N.try_call("dgv2_gemm_stream_tn", *args)):
        N.call("dgv2_bmm_tn", *args)


def bmm_tn_cat_call(*args):
    """dgv2_bmm_tn_cat(*args), on dgv2_gemm_stream_tn_cat where the switch is on and the entry covers the geometry."""
    if not (_stream_wanted(args[5]) and N.try_call("dgv2_gemm_stream_tn_cat", *args)):
        N.call("dgv2_bmm_tn_cat", *args)


def _bmm_nn_raw(x3, w3, out_dtype, bias=None, act=0, alpha=0.2, scale=1.0, sq=None, row_scale=None, resid=None, head=None):
    """x3 [B,P,I]; w3 [Bw,O,I] (Bw = B or 1) same dtype -> [B,P,O]; optional fused
    bias (fp32 [O]) + leaky-ReLU epilogue.  sq = _sq_args(): sum-of-squares partials where the kernel has them.
    head = [hw [B,2,O] bf16, None]: where the kernel can, the contraction of the level's two output heads on THIS output
    leaves from the same launch (dgv2_modconv_pe_fwd_head): head[1] then holds it, fp32 [B,P,2]; else it stays None."""
    B, P, I = x3.shape
    Bw, O, _ = w3.shape
    N.check(x3, w3, bias)
    y = torch.empty((B, P, O), device=x3.device, dtype=out_dtype)
    if I <= 4 and Bw == B and bias is None and act == 0 and sq is None and row_scale is None and out_dtype == x3.dtype:
        # contraction over the <= 4 channels of the output heads (their data gradient): outer-product stream
        r = None if resid is None else resid.contiguous().to(out_dtype)
        if N.try_call("dgv2_bmm_nn_small", N.ptr(y), N.ptr(x3), N.ptr(w3), N.ptr(r), B, P, I, O, _dt(x3), N.stream()):
            return y
    if (resid is None and _PE_FWD and Bw == B and x3.dtype == torch.bfloat16 and out_dtype == torch.bfloat16
            and P >= _PE_FREE_MINP.get((I, O), 1 << 30)):
        # streaming shapes of the two top levels: sample-walking kernel without a PE part
        if (head is not None and _HEAD_FWD and head[0].dtype == torch.bfloat16 and tuple(head[0].shape) == (B, 2, O)
                and head[0].is_contiguous()):
            hd = torch.empty((B, P, 2), device=x3.device, dtype=torch.float32)
            if N.try_call("dgv2_modconv_pe_fwd_head", N.ptr(y), N.ptr(x3), None, N.ptr(w3), B, P, I, 0, O, N.ptr(row_scale),
                          N.ptr(bias), act, alpha, scale, _dt(x3), *_sq_tail(sq), N.ptr(head[0]), N.ptr(hd), N.stream()):
                head[1] = hd
                return y
        N.call("dgv2_modconv_pe_fwd_sq", N.ptr(y), N.ptr(x3), None, N.ptr(w3), B, P, I, 0, O, N.ptr(row_scale),
               N.ptr(bias), act, alpha, scale, _dt(x3), *_sq_tail(sq), N.stream())
        return y
    # routing onto the stream engine differs at B == Bw == 1 only: a plain call counts the single weight as per-sample,
    # a call with sq / row_scale / resid as batch-shared (its wstride is 0: the generic engine)
    plain = sq is None and row_scale is None and resid is None
    if resid is not None:
        resid = resid.contiguous().to(out_dtype)
        N.check(resid)
    bmm_nn_sq_call(N.ptr(y), N.ptr(x3), N.ptr(w3), B, P, I, O, I, O, 0 if Bw == 1 else O * I, N.ptr(row_scale),
                   N.ptr(bias), act, alpha, scale, N.ptr(resid), _dt(x3), N.dtype_code(y), *_sq_tail(sq), N.stream(),
                   per_sample=Bw == B if plain else Bw != 1)
    return y


def _bmm_tn_raw(gy3, x3):
    """gy3 [B,P,O], x3 [B,P,I] -> fp32 [B,O,I]."""
    B, P, O = gy3.shape
    I = x3.shape[2]
    N.check(gy3, x3)
    gw = torch.empty((B, O, I), device=x3.device, dtype=torch.float32)
    bmm_tn_call(N.ptr(gw), N.ptr(gy3), N.ptr(x3), B, P, I, O, O, I, _dt(x3), N.stream())
    return gw


class _ModGemm(Function):
    """y[b,p,o] = sum_i x[b,p,i] w[b,o,i]; w is an fp32 master ([B,O,I] or shared [1,O,I])."""

    @staticmethod
    def forward(ctx, x, w, out_dtype):
        shp = x.shape
        x3 = x.contiguous().reshape(shp[0], -1, shp[-1])
        wc = _values(w, x.dtype)
        y = _bmm_nn_raw(x3, wc, out_dtype)
        ctx.save_for_backward(x3, wc)
        ctx.cfg = (shp, w.shape[0] == 1)
        return y.reshape(*shp[:-1], w.shape[1])

    @staticmethod
    def backward(ctx, gy):
        x3, wc = ctx.saved_tensors
        shp, shared = ctx.cfg
        gy3 = gy.contiguous().reshape(x3.shape[0], -1, wc.shape[1]).to(x3.dtype)
        gx = gw = None
        if ctx.needs_input_grad[0]:
            wt = wc.transpose(1, 2).contiguous()
            gx = _bmm_nn_raw(gy3, wt, x3.dtype).reshape(shp)
        if ctx.needs_input_grad[1]:
            if shared:
                gw = _bmm_tn_raw(gy3.reshape(1, -1, gy3.shape[2]), x3.reshape(1, -1, x3.shape[2]))
            else:
                gw = _bmm_tn_raw(gy3, x3)
        return gx, gw, None


def mod_gemm(x, w, out_dtype=None):
    return _ModGemm.apply(x, w, x.dtype if out_dtype is None else out_dtype)


class _ModGemmAct(Function):
    """lrelu(x @ w^T + b) * scale with the bias/activation fused into the GEMM epilogue
    (reference: ModConv2d followed by FusedLeakyReLU, gans/models/dusty_v2.py:161-170)."""

    @staticmethod
    def forward(ctx, x, w, bias, alpha, scale):
        shp = x.shape
        x3 = x.contiguous().reshape(shp[0], -1, shp[-1])
        wc = _values(w, x.dtype)
        out = _bmm_nn_raw(x3, wc, x.dtype, bias.detach().float().contiguous(), 3, alpha, scale)
        ctx.save_for_backward(x3, wc, out)
        ctx.cfg = (shp, w.shape[0] == 1, alpha, scale, bias.numel())
        return out.reshape(*shp[:-1], w.shape[1])

    @staticmethod
    def backward(ctx, gy):
        x3, wc, out = ctx.saved_tensors
        shp, shared, alpha, scale, size_b = ctx.cfg
        gpre, gb = _BiasActBackward.apply(gy.contiguous().reshape(out.shape), out, True, alpha, scale, 1, size_b)
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = _bmm_nn_raw(gpre, wc.transpose(1, 2).contiguous(), x3.dtype).reshape(shp)
        if ctx.needs_input_grad[1]:
            if shared:
                gw = _bmm_tn_raw(gpre.reshape(1, -1, gpre.shape[2]), x3.reshape(1, -1, x3.shape[2]))
            else:
                gw = _bmm_tn_raw(gpre, x3)
        return gx, gw, gb, None, None


def mod_gemm_act(x, w, bias, alpha=0.2, scale=math.sqrt(2.0)):
    return _ModGemmAct.apply(x, w, bias, float(alpha), float(scale))


class _ModGemmCatAct(Function):
    """Level-input conv with a batch-shared positional encoding (dgv2_bmm_nn_cat_sq / dgv2_bmm_tn_cat):
    out = lrelu([xa | xs] @ w^T + b) * scale, xa [B,H,W,Ka] per sample (or None), xs [1,H,W,Ks] shared."""

    @staticmethod
    def forward(ctx, xa, xs, w, bias, alpha, scale):
        B, O = w.shape[0], w.shape[1]
        _, H, W_, Ks = xs.shape
        Ka = 0 if xa is None else xa.shape[3]
        xs = xs.contiguous()
        xa = None if xa is None else xa.contiguous()
        wc = w.detach().to(xs.dtype).contiguous()
        bias32 = bias.detach().float().contiguous()
        N.check(xa, xs, wc, bias32)
        out = torch.empty((B, H, W_, O), device=xs.device, dtype=xs.dtype)
        bmm_nn_cat_sq_call(N.ptr(out), N.ptr(xa), N.ptr(xs), N.ptr(wc), B, H * W_, Ka, Ks, O, None, N.ptr(bias32),
                           3, alpha, scale, _dt(xs), _dt(xs), None, 0, None, N.stream())
        ctx.save_for_backward(xa, xs, wc, out)
        ctx.cfg = (alpha, scale, Ka, Ks)
        return out

    @staticmethod
    def backward(ctx, gy):
        xa, xs, wc, out = ctx.saved_tensors
        alpha, scale, Ka, Ks = ctx.cfg
        B, H, W_, O = out.shape
        gpre, gb = _BiasActBackward.apply(gy.contiguous(), out, True, alpha, scale, 1, O)
        gxa = gw = None
        g3 = gpre.reshape(B, H * W_, O)
        if xa is not None and ctx.needs_input_grad[0]:
            wt = wc[:, :, :Ka].transpose(1, 2).contiguous()  # only the activation channels need a data gradient
            gxa = _bmm_nn_raw(g3, wt, xa.dtype).reshape(xa.shape)
        if ctx.needs_input_grad[2]:
            gw = torch.empty((B, O, Ka + Ks), device=out.device, dtype=torch.float32)
            bmm_tn_cat_call(N.ptr(gw), N.ptr(g3), N.ptr(xa), N.ptr(xs), B, H * W_, Ka, Ks, O, _dt(xs), N.stream())
        return gxa, None, gw, gb, None, None


def mod_gemm_cat_act(xa, xs, w, bias, alpha=0.2, scale=math.sqrt(2.0)):
    return _ModGemmCatAct.apply(xa, xs, w, bias, float(alpha), float(scale))


def _values(w, dtype):
    """Compute-dtype VALUES of a conv weight; a weight-bank handle has none (its prepared copies did not match
    this call: wrong dtype, or a second-order pass that must run with the bank off)."""
    if getattr(w, "_dgv2_bank", None) is not None:   # (native.conv: what marks a handle)
        raise RuntimeError("conv weight handle without values: run this pass without the weight bank "
                           "(Discriminator.forward(double_backward=True))")
    # one conversion per weight tensor and pass: the second-order passes of R1 (bank off) use each effective weight in
    # the forward conv, the data gradient and the conv of the double backward -- the copy rides on the tensor object
    # (a fresh `weight * gain` per forward; `_version` guards a parameter used directly)
    if w.dtype == dtype and w.is_contiguous():
        return w.detach()
    return versioned(w, "_dgv2_vals", lambda: w.detach().to(dtype).contiguous(), ok=lambda v: v.dtype == dtype)


__all__ = ["bmm_nn_sq_call", "bmm_nn_cat_sq_call", "bmm_tn_call", "bmm_tn_cat_call", "mod_gemm", "mod_gemm_act",
           "mod_gemm_cat_act", "_PE_FREE_MINP", "_bmm_nn_raw"]
