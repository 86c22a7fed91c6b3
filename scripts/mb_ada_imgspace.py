"""dgv2_ada_apply_img against dgv2_ada_apply at B = 64 one-channel 64x512 images: us per launch, forward and transpose, for the
parent's 32 taps, the folded 74 taps (LDS kernel and, with DGV2_NO_ADA_LDS=1 in the environment, the generic kernel), with and
without the mask / noise terms; then the fold and the whole AdaptiveAugment.forward with and without the image-space stages.
usage: mb_ada_imgspace.py"""
import os, sys, torch
sys.path[:0] = ["dusty-gan-v2_amd"]
from gans.models.ops import native as nat
N = nat.N
def t(fn, n=50):
    fn(); fn(); fn(); torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3
B, H, W = 64, 64, 512
x = torch.randn(B, H, W, device="cuda"); y = torch.empty_like(x); eps = torch.randn_like(x)
Ay = torch.randn(B, H, H, device="cuda")
off = torch.randint(0, W, (B,), device="cuda", dtype=torch.int32); sgn = (torch.randint(0, 2, (B,), device="cuda", dtype=torch.int32) * 2 - 1)
a = torch.randn(B, device="cuda"); c = torch.randn(B, device="cuda"); sigma = torch.rand(B, device="cuda")
cut = torch.cat([torch.rand(B, 2, device="cuda"), torch.full((B, 2), 0.5, device="cuda")], 1).contiguous()
print("kernel: " + ("generic (DGV2_NO_ADA_LDS)" if os.environ.get("DGV2_NO_ADA_LDS") else "LDS"), flush=True)
for K in (32, 74):
    kx = torch.randn(B, K, device="cuda")
    for name, extra in (("plain", (None, None, None)), ("mask+noise", (cut, sigma, eps))):
        out = []
        for tr in (0, 1):
            if K <= 64 and name == "plain":
                us = t(lambda: N.call("dgv2_ada_apply", N.ptr(y), N.ptr(x), N.ptr(Ay), N.ptr(kx), N.ptr(off), N.ptr(sgn), N.ptr(a), N.ptr(c), B, H, W, K, tr, N.stream()))
                out.append(f"apply {'T' if tr else 'F'} {us:6.1f} us")
            us = t(lambda: N.call("dgv2_ada_apply_img", N.ptr(y), N.ptr(x), N.ptr(Ay), N.ptr(kx), N.ptr(off), N.ptr(sgn), N.ptr(a), N.ptr(c), *[N.ptr(v) for v in extra], B, H, W, K, tr, N.stream()))
            out.append(f"apply_img {'T' if tr else 'F'} {us:6.1f} us")
        print(f"B={B} 64x512 K={K} {name}: " + "   ".join(out), flush=True)
from gans.augment.adaptive_augment import AdaptiveAugment
geo = dict(lr_flip=1, ud_flip=1, int_trans=1, iso_scale=1, frac_trans=1, brightness=1, contrast=1, luma_flip=1, hue=1, saturation=1)
x4 = x.reshape(B, 1, H, W)
with torch.no_grad():
    for name, img in (("off", {}), ("on", dict(imgfilter=1, noise=1, cutout=1))):
        A = AdaptiveAugment(p_init=0.6, **geo, **img).cuda()
        print(f"AdaptiveAugment.forward, B = 64, image-space stages {name}: {t(lambda: A(x4)):6.1f} us", flush=True)
    A = AdaptiveAugment(p_init=0.6, **geo, imgfilter=1).cuda()
    kx = torch.randn(B, 32, device="cuda"); g = torch.rand(B, 4, device="cuda") + 0.5
    print(f"dgv2_ada_fold, B = 64: {t(lambda: nat.ada_fold(Ay, kx, off, sgn, c, g, A.Hz_fbank, W)):6.1f} us", flush=True)
