"""The residual blocks' 1x1 skip conv at the benchmark's eight shapes (four blocks, G body B = 64 and D body 2B = 128):
forward (+ residual) and data gradient, the direct engine (conv_pipe_kernel via dgv2_conv_direct_fwd / _dgrad) against conv1x1.hip's
streaming GEMM in the same process.  us per launch, GB/s against the HBM floor's byte count (operand read + residual
read + result written, bf16) and the fraction of the 6.3 TB/s a float4 copy reaches.

Each timing is one hipGraph of REPS launches replayed ROUNDS times, the two engines alternating; the launches walk over
enough operand sets that a set is not met again before ~512 MB of other traffic passed (the small blocks would otherwise
run out of the 256 MB Infinity Cache).  Reported: the median round."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dusty-gan-v2_amd")]
import torch

from gans.models.ops import native
from gans.models.ops.native import conv as nconv

REPS, ROUNDS, HBM = 16, 5, 6.3e12
BLOCKS = [(32, 256, 32, 64), (16, 128, 64, 128), (8, 64, 128, 256), (4, 32, 256, 512)]   # (H, W, C, O) behind blur_down
GEOM = native.ConvGeom(1, 1, 1, 0, True)
BF = torch.bfloat16


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
    print(f"{'form':6s} {'B':>4s} {'HxW':>7s} {'C->O':>9s} {'direct us':>10s} {'1x1 us':>8s} {'floor us':>9s} {'1x1 GB/s':>9s} "
          f"{'of 6.3TB/s':>10s} {'x floor':>8s} {'speed-up':>9s}")
    for B in (64, 128):
        for H, W, C, O in BLOCKS:
            P = H * W
            for form in ("fwd", "dgrad"):
                nbytes = 2 * B * P * (C + 2 * O if form == "fwd" else O + C)
                nsets = max(2, min(16, -(-(512 << 20) // nbytes)))
                sets = []
                for _ in range(nsets):
                    w = (torch.randn(O, 1, 1, C, device="cuda") * C ** -0.5).to(BF)
                    sets.append(dict(x=torch.randn(B, H, W, C, device="cuda").to(BF), gy=torch.randn(B, H, W, O, device="cuda").to(BF),
                                     ry=torch.randn(B, H, W, O, device="cuda").to(BF), w=w,
                                     wt=w.reshape(O, C).t().reshape(C, 1, O).contiguous()))
                if form == "fwd":
                    fn = lambda t: nconv._conv_fwd_raw(t["x"], t["w"], GEOM, resid=t["ry"])
                else:
                    fn = lambda t: nconv._conv_dgrad_raw(t["gy"], None, GEOM, (B, H, W, C), wt=t["wt"])
                graphs = {}
                for on in (False, True):
                    nconv._CONV1X1 = on
                    graphs[on] = graph_of(fn, sets)
                times = {False: [], True: []}
                for _ in range(ROUNDS):
                    for on in (False, True):
                        times[on].append(time_graph(graphs[on]))
                old, new = statistics.median(times[False]), statistics.median(times[True])
                floor = nbytes / HBM
                print(f"{form:6s} {B:4d} {f'{H}x{W}':>7s} {C:4d}->{O:<4d} {old * 1e6:10.1f} {new * 1e6:8.1f} {floor * 1e6:9.1f} "
                      f"{nbytes / new / 1e9:9.0f} {nbytes / new / HBM:10.2f} {new / floor:8.2f} {old / new:9.2f}")
                del graphs, sets
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
