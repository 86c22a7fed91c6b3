"""The per-sample-weight contractions of the generator's levels 0 and 1 at the benchmark's shapes (B = 64, bf16): the
generic engines (gemm_nn_kernel / gemm_tn_kernel) against gemm_stream.hip in the same process, through the calls the
layers make (modgemm.bmm_*_call with the module flag flipped).

Seven instances -- the rows of the step listing these kernels appear in:
  nn_cat  P 128  K 0+512    O 512   level 0 conv1 forward (bias + leaky ReLU + row scale + partials)
  nn_cat  P 512  K 512+512  O 256   level 1 conv1 forward (same epilogue)
  nn      P 512  K 256      O 512   level 1 conv1 data gradient
  tn_cat  P 512  O 256  J 512+512   level 1 conv1 weight gradient
  tn_cat  P 128  O 512  J 0+512     level 0 conv1 weight gradient
  tn      P 128  O 512  J 512       level 0 conv2 weight gradient
  tn      P 512  O 256  J 256       level 1 conv2 weight gradient

Each timing is one hipGraph of REPS launches replayed once, the two engines alternating, REPEATS times each; the launches
walk over enough operand sets that a set is not met again before ~512 MB of other traffic passed.  Printed per engine:
min and max of the repeats (us per launch); then the speed-up of the minima, whether the new engine is slower than the
generic one by more than the larger of the two spreads, TFLOP/s, and the byte floor (operands read once + result
written, the batch-shared PE counted once) at 6.3 TB/s with the fraction of it the new engine reaches."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dusty-gan-v2_amd")]
import torch

import dgv2_native as N
from gans.models.ops.native import modgemm

REPS, REPEATS, HBM, B = 16, 3, 6.3e12, 64
BF = torch.bfloat16
SQ_CAP = 8192

INSTANCES = [("nn_cat", 128, 0, 512, 512), ("nn_cat", 512, 512, 512, 256), ("nn", 512, 256, 0, 512),
             ("tn_cat", 512, 512, 512, 256), ("tn_cat", 128, 0, 512, 512), ("tn", 128, 512, 0, 512), ("tn", 512, 256, 0, 256)]


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, device="cuda") * scale).to(BF)


def operand_set(form, P, Ka, Ks, O):
    K = Ka + Ks
    if form == "nn_cat":
        return dict(xa=rnd(B, P, Ka) if Ka else None, xs=rnd(P, Ks), w=rnd(B, O, K, scale=K ** -0.5),
                    y=torch.empty(B, P, O, device="cuda", dtype=BF), rs=torch.rand(O, device="cuda") + 0.5,
                    b=torch.randn(O, device="cuda"), sq=torch.empty(SQ_CAP, device="cuda"), used=ctypes.c_int(0))
    if form == "nn":
        return dict(x=rnd(B, P, K), w=rnd(B, O, K, scale=K ** -0.5), y=torch.empty(B, P, O, device="cuda", dtype=BF))
    return dict(gy=rnd(B, P, O), xa=rnd(B, P, Ka) if Ka else None, xs=rnd(P, Ks) if Ks else None,
                gw=torch.empty(B, O, K, device="cuda"))


def launch(form, P, Ka, Ks, O, t):
    st = N.stream()
    if form == "nn_cat":
        modgemm.bmm_nn_cat_sq_call(N.ptr(t["y"]), N.ptr(t["xa"]), N.ptr(t["xs"]), N.ptr(t["w"]), B, P, Ka, Ks, O, N.ptr(t["rs"]),
                                   N.ptr(t["b"]), 3, 0.2, 2.0 ** 0.5, N.BF16, N.BF16, N.ptr(t["sq"]), SQ_CAP,
                                   ctypes.addressof(t["used"]), st)
    elif form == "nn":
        modgemm.bmm_nn_sq_call(N.ptr(t["y"]), N.ptr(t["x"]), N.ptr(t["w"]), B, P, Ka, O, Ka, O, O * Ka, None, None, 0, 0.2, 1.0,
                               None, N.BF16, N.BF16, None, 0, None, st)
    elif form == "tn_cat":
        modgemm.bmm_tn_cat_call(N.ptr(t["gw"]), N.ptr(t["gy"]), N.ptr(t["xa"]), N.ptr(t["xs"]), B, P, Ka, Ks, O, N.BF16, st)
    else:
        modgemm.bmm_tn_call(N.ptr(t["gw"]), N.ptr(t["gy"]), N.ptr(t["xa"]), B, P, Ka, O, O, Ka, N.BF16, st)


def traffic(form, P, Ka, Ks, O):
    K = Ka + Ks
    if form in ("nn_cat", "nn"):
        return 2 * (B * P * Ka + P * Ks + B * O * K + B * P * O)
    return 2 * (B * P * O + B * P * Ka + P * Ks) + 4 * B * O * K


def graph_of(fn, sets):
    fn(sets[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(REPS):
            fn(sets[i % len(sets)])
    return g


def time_graph(g):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e-3 / REPS


def main():
    print("# python scripts/mb_gemm_lowlevels.py on one MI355X (B = 64, bf16; us per launch, min .. max of three graph replays "
          "per engine, alternating)")
    print(f"{'form':7s} {'P':>4s} {'K / J':>8s} {'O':>4s} | {'generic us min..max':>20s} | {'stream us min..max':>19s} | {'speed-up':>8s} "
          f"{'slower?':>8s} {'TFLOP/s':>8s} {'floor us':>9s} {'of floor':>9s}")
    for form, P, Ka, Ks, O in INSTANCES:
        nbytes = traffic(form, P, Ka, Ks, O)
        flops = 2.0 * B * P * (Ka + Ks) * O
        nsets = max(2, min(16, -(-(512 << 20) // nbytes)))
        sets = [operand_set(form, P, Ka, Ks, O) for _ in range(nsets)]
        fn = lambda t: launch(form, P, Ka, Ks, O, t)
        graphs = {}
        for on in (False, True):
            modgemm._GEMM_STREAM = on
            graphs[on] = graph_of(fn, sets)
        for on in (False, True):   # one untimed replay each
            time_graph(graphs[on])
        times = {False: [], True: []}
        for _ in range(REPEATS):
            for on in (False, True):
                times[on].append(time_graph(graphs[on]))
        old, new = times[False], times[True]
        spread = max(max(old) - min(old), max(new) - min(new))
        slower = "YES" if min(new) > min(old) + spread else "no"
        floor = nbytes / HBM
        print(f"{form:7s} {P:4d} {f'{Ka}+{Ks}':>8s} {O:4d} | {min(old) * 1e6:9.1f} ..{max(old) * 1e6:8.1f} | {min(new) * 1e6:8.1f} ..{max(new) * 1e6:8.1f} | "
              f"{min(old) / min(new):8.2f} {slower:>8s} {flops / min(new) / 1e12:8.1f} {floor * 1e6:9.1f} {floor / min(new):9.2f}")
        del graphs, sets
        torch.cuda.empty_cache()
    modgemm._GEMM_STREAM = True


if __name__ == "__main__":
    main()
