#!/usr/bin/env python3
"""Generate tests/golden/conv_direct_digests.json: a sha256 of the output bytes of every case of
tests/conv_direct_cases.py on random operands (needs the MI355X and the built libdgv2.so).

    make && python tests/golden/make_conv_direct_golden.py [OUT.json]

The committed file was recorded with the library of ABI 58, the last one whose direct conv engine was driven by tap
lists (dgv2_conv_taps*): tests/test_gpu_conv_direct.py holds the geometry entries of ABI 59 to the same bits.  The
kernels store their results (no atomics), so two recordings agree; the script checks that by running every case twice.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
for p in (os.path.join(ROOT, "dusty-gan-v2_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, os.path.abspath(p))
OUT = os.path.join(HERE, "conv_direct_digests.json")


def main():
    import torch

    import conv_direct_cases as cc
    import dgv2_native as N
    from gans.models.ops import native
    out = {}
    for case in cc.CASES:
        first = [cc.digest(t) for t in cc.run(native, case, False)[0]]
        again = [cc.digest(t) for t in cc.run(native, case, False)[0]]
        if first != again:
            raise SystemExit(f"{case[0]}: two runs of the same call disagree")
        for i, d in enumerate(first):
            out[f"{case[0]}/{i}"] = d
    torch.cuda.synchronize()
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"ABI {N.lib.dgv2_abi_version()}: {len(out)} digests -> {path}")


if __name__ == "__main__":
    main()
