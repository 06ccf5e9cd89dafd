"""Times the mix-augmentation stage (consistencytta_amd.data.collate) at the training batch shapes: one loader batch of
6 clips of 10.24 s (3 mixtures) and the fused micro-batch of 30 clips in 5 groups (15 mixtures).  Prints one JSON line
per shape with the device-event time per call (median over --iters calls, after --warmup).  Kernel times come from a
separate run under `rocprofv3 --kernel-trace --stats -- python tools/mix_bench.py`.

The bytes and FLOPs printed are what the algorithm needs, computed from the shapes: every source sample is read once
by the frame-energy kernel (frames overlap by half: 2x) and once per pair it belongs to, each mixture is written,
read and written again by the normalisation; the FFT costs ~5 N log2 N flops per frame."""
import argparse
import json
import math
import os
import random
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from consistencytta_amd import data  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=163840)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mix_bench needs a GPU"
    L, n_fft = a.samples, 2048
    frames = (L - n_fft) // (n_fft // 2) + 1
    for B, groups in ((6, 1), (30, 5)):
        g = torch.Generator().manual_seed(B)
        wav = ((torch.rand(B, L, generator=g) - 0.5) * torch.linspace(0.05, 1.0, B)[:, None]).cuda()
        caps = ["clip %d" % i for i in range(B)]
        random.seed(0)
        n = B // 2
        out = torch.empty(B + n, L, device="cuda")
        for _ in range(a.warmup):
            data.collate(caps, wav, out=out, groups=groups)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            data.collate(caps, wav, out=out, groups=groups)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        times.sort()
        nbytes = 4 * (2 * B * L + B * L * 2 + 2 * n * L + 3 * n * L)   # energy reads, row copy, pair reads, mix + normalise
        flops = B * frames * (5 * n_fft * math.log2(n_fft) + 4 * n_fft) + 3 * n * L
        print(json.dumps({"batch": B, "groups": groups, "mixtures": n, "samples": L, "us_per_collate_median": round(times[len(times) // 2], 1),
                          "us_min": round(times[0], 1), "mbytes_needed": round(nbytes / 1e6, 2), "gflop": round(flops / 1e9, 3)}))


if __name__ == "__main__":
    main()
