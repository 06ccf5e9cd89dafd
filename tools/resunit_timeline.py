#!/usr/bin/env python3
"""Per-workgroup phase timeline of one fused ResBlock-unit launch (ctta_conv_debug_stamps): staging, conv1, intermediate
write, conv2, epilogue, and the gap to the next workgroup's entry on the same CU.
usage: resunit_timeline.py C K DIL [batch]      at the vocoder's stage length for C (512: 5121, 256: 20484, 128: 40960,
                                                64: 81920, 32: 163840)
       resunit_timeline.py --table [batch]      k = 3 (d = 1) and k = 11 (d = 5) at all five widths: the table kept in
                                                profiles/resunit_phases.txt"""
import os
import sys
from collections import defaultdict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from consistencytta_amd import _native as N  # noqa: E402

LEN = {512: 5121, 256: 20484, 128: 40960, 64: 81920, 32: 163840}
MHz = float(os.environ.get("TICK_MHZ", "0"))      # ticks of s_memtime per us; 0 = estimated from the launch's event time
L = N.lib()


def pct(v):
    return (v.mean(),) + tuple(np.percentile(v, [10, 50, 90]))


def overlap_share(intervals):
    """share of the time in which at least one of the intervals is open during which two or more are"""
    ev = sorted([(a, 1) for a, _ in intervals] + [(b, -1) for _, b in intervals])
    cur, last, any_, two = 0, ev[0][0], 0.0, 0.0
    for tt, d in ev:
        if cur >= 1:
            any_ += tt - last
        if cur >= 2:
            two += tt - last
        last, cur = tt, cur + d
    return two / max(any_, 1.0)


def timeline(C, k, dil, B):
    Lw = LEN[C]
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(B, Lw, C, generator=g) * 0.5).to(torch.bfloat16).to("cuda:0")
    out = torch.empty_like(x)
    w1, w2 = [(torch.randn(C * k * C, generator=g) * (C * k) ** -0.5).to(torch.bfloat16).to("cuda:0") for _ in range(2)]
    b1, b2 = [(torch.randn(C, generator=g) * 0.1).to("cuda:0") for _ in range(2)]

    def run():
        N.check(L.ctta_resunit_conv1d(N.ptr(x), B, Lw, C, k, dil, N.ptr(w1), N.ptr(b1), N.ptr(w2), N.ptr(b2), 0.1, N.ptr(out), 0,
                                      1.0, 0.0, N.stream_ptr()))

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    buf = torch.zeros((1 << 16) * 8, dtype=torch.int64, device="cuda:0")
    L.ctta_conv_debug_stamps(buf.data_ptr())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    L.ctta_conv_debug_stamps(None)
    s = buf.cpu().numpy().reshape(-1, 8)
    s = s[s[:, 1] != 0]
    hw = s[:, 0] & 0xFFFFFFFF
    xcc = (s[:, 0] >> 32) & 0xF
    cu_key = (xcc << 16) | (hw & 0xFF00)
    t = s[:, 1:7].astype(np.float64)
    by = defaultdict(list)
    for i, key in enumerate(cu_key.tolist()):
        by[key].append(i)
    # the counters of different XCCs do not share an origin: spans are taken per CU.  The tick rate is not the documented
    # 100 MHz on every box, so by default it is the median per-CU span (first entry .. last store) over the event time
    ev_us = e0.elapsed_time(e1) * 1e3
    span = float(np.median([t[idx, 5].max() - t[idx, 0].min() for idx in by.values()]))
    mhz = MHz or span / ev_us
    us = lambda v: v / mhz
    print("C%d k%d d%d B%d: launch %.1f us by events; %d tiles on %d (xcc, cu) keys; median span per CU %.0f ticks, %.2f ticks per us%s"
          % (C, k, dil, B, ev_us, len(s), len(by), span, mhz, "" if MHz else " (estimated)"))
    names = ("stage", "conv1", "mid write", "conv2", "epilogue")
    for i, name in enumerate(names):
        print("  %-10s mean %7.2f us  p10 %7.2f  p50 %7.2f  p90 %7.2f" % ((name,) + pct(us(t[:, i + 1] - t[:, i]))))
    print("  %-10s mean %7.2f us  p10 %7.2f  p50 %7.2f  p90 %7.2f" % (("whole",) + pct(us(t[:, 5] - t[:, 0]))))
    conc, gaps, share = [], [], []
    for key, idx in by.items():
        ev = sorted([(t[i, 0], 1) for i in idx] + [(t[i, 5], -1) for i in idx])
        cur, last, area = 0, ev[0][0], 0.0
        for tt, d in ev:
            area += cur * (tt - last)
            last, cur = tt, cur + d
        conc.append(area / max(ev[-1][0] - ev[0][0], 1))
        # exit-to-entry gap: every tile entered after some tile of this CU has issued its last store, against the
        # latest such exit (the slot it took over; a tile of a walking workgroup follows its own predecessor)
        ends = np.sort(t[idx, 5])
        for i in idx:
            j = np.searchsorted(ends, t[i, 0], side="right")
            if j > 0:
                gaps.append(t[i, 0] - ends[j - 1])
        share.append(overlap_share([(t[i, 0], t[i, 1]) for i in idx]))
    if gaps:
        print("  %-10s mean %7.2f us  p10 %7.2f  p50 %7.2f  p90 %7.2f" % (("exit-entry",) + pct(us(np.array(gaps)))))
    print("  tiles per CU: min %d max %d; mean resident workgroups per CU (entry .. last store issued) %.2f"
          % (min(len(v) for v in by.values()), max(len(v) for v in by.values()), float(np.mean(conc))))
    print("  staging of two or more workgroups of a CU at the same time: %.0f %% of the CU's staging time (mean over CUs)"
          % (100 * float(np.mean(share))), flush=True)


if sys.argv[1] == "--table":
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    for C in (512, 256, 128, 64, 32):
        for k, dil in ((3, 1), (11, 5)):
            timeline(C, k, dil, B)
else:
    timeline(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 32)
