"""Weight-gradient routes of the VAE decoder's last level (1024 x 64 at batch 4), timed on one box in one call:

  * the implicit 3x3 kernel at width 64 (wgrad_implicit_w64_kernel) in its three operand forms -- dY^T (the transposed copy
    included), dY in place with split slabs + scatter, one split added straight into the gradient -- against
  * the copies route it replaces at that width: ctta_im2col_t + ctta_transpose_bf16 + ctta_conv_gemm + ctta_wgrad_rowsum +
    scatter,

for the layers 128 -> 128 and 256 -> 128, and for the x2 upsampling convolution 256 -> 256 into 1024 x 64 (copies route,
which knows `upsample`, against a materialised x2 input read by the implicit kernel).  Warm-up, then `--reps` timed
replays per route with device events, the routes alternating; prints one table.

    python tools/vae_wgrad_bench.py [--batch 4] [--reps 20] [--out profiles/vae_wgrad.txt]
"""
import argparse
import ctypes
import functools
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from consistencytta_amd import _native as N  # noqa: E402

DEV = "cuda:0"


def rup(a, b):
    return (a + b - 1) // b * b


def splits_for(tiles, M, cap=16, floor=256, target=256):
    S = 1
    while tiles * S < target and S < cap and M // (2 * S) >= floor:
        S *= 2
    return S


class Layer:
    """One 3x3 convolution's weight-gradient problem: x (B, H, W, Cin) or, ups, (B, H/2, W/2, Cin); dy (B, H, W, Cout)."""

    def __init__(self, B, H, W, Cin, Cout, ups):
        g = torch.Generator(device=DEV).manual_seed(1)
        self.B, self.H, self.W, self.Cin, self.Cout, self.ups = B, H, W, Cin, Cout, ups
        hs, ws = (H // 2, W // 2) if ups else (H, W)
        self.x = (torch.rand(B, hs, ws, Cin, generator=g, device=DEV) * 2 - 1).to(torch.bfloat16)
        self.dy = (torch.rand(B, H, W, Cout, generator=g, device=DEV) * 2 - 1).to(torch.bfloat16)
        self.M, self.K = B * H * W, 9 * Cin
        self.ld = rup(self.K + 1, 4)
        self.ro = (torch.arange(Cout, dtype=torch.int32) * self.K).to(DEV)
        self.gw = torch.zeros(Cout, self.K, device=DEV)
        self.gb = torch.zeros(Cout, device=DEV)
        self.bufs = {}

    def buf(self, name, shape, dtype):
        if name not in self.bufs:
            self.bufs[name] = torch.empty(shape, dtype=dtype, device=DEV)
        return self.bufs[name]

    def scatter(self, slabs, S):
        L, st = N.lib(), N.stream_ptr()
        N.check(L.ctta_wgrad_scatter_rows_bias(N.ptr(slabs), S, self.Cout * self.ld, self.ld, self.K, self.Cout, N.ptr(self.ro), None,
                                               N.ptr(self.gw), self.K, self.Cout, None, N.ptr(self.gb), 0, st))

    def x_full(self):
        """The implicit kernel's input: x itself, or (ups) the materialised nearest x2 copy -- part of that route's time."""
        if not self.ups:
            return self.x
        up = self.buf("xup", (self.B, self.H, self.W, self.Cin), torch.bfloat16)
        N.check(N.lib().ctta_upsample2_nearest(N.ptr(self.x), N.ptr(up), self.B, self.H // 2, self.W // 2, self.Cin, N.stream_ptr()))
        return up

    def copies(self):
        L, st = N.lib(), N.stream_ptr()
        S = splits_for(((self.K + 127) // 128) * ((self.Cout + 127) // 128), self.M)
        mp = rup(self.M, 64 * S)
        seg = mp // S
        q = self.buf("q", (self.K + 1, mp), torch.bfloat16)
        pt = self.buf("pt%d" % mp, (self.Cout, mp), torch.bfloat16)
        slabs = self.buf("slabs%d" % S, (S, self.Cout, self.ld), torch.float32)
        N.check(L.ctta_transpose_bf16(N.ptr(self.dy), 0, self.M, self.Cout, self.Cout, 0, N.ptr(pt), 0, mp, 1, st))
        N.check(L.ctta_im2col_t(N.ptr(self.x), self.Cin, self.B, self.H, self.W, int(self.ups), self.H, self.W, 3, 3, 1, 1, 1, 1, N.ptr(q),
                                mp, 0, st))
        d = N.ConvDesc()
        d.kh = d.kw = d.stride_h = d.stride_w = d.dil_h = d.dil_w = 1
        d.alpha = 1.0
        d.x0, d.c0, d.x_stride = pt.data_ptr(), seg, mp
        d.batch, d.hi, d.wi, d.ho, d.wo = 1, self.Cout, 1, self.Cout, 1
        d.w, d.k_pad, d.n = q.data_ptr(), mp, self.K
        d.out, d.ldc, d.out_f32 = slabs.data_ptr(), self.ld, 1
        d.groups, d.x_group_stride, d.w_group_stride, d.out_group_stride = S, seg, seg, self.Cout * self.ld
        N.check(L.ctta_conv_gemm(ctypes.byref(d), st))
        N.check(L.ctta_wgrad_rowsum(N.ptr(pt), self.Cout, mp, self.M, S, self.H * self.W, 0, N.ptr(slabs), self.Cout * self.ld, self.ld,
                                    self.K, st))
        self.scatter(slabs, S)
        return "copies (S=%d)" % S

    def _implicit_S(self, cap=16, target=256):
        return splits_for(((self.Cout + 63) // 64) * ((self.Cin + 63) // 64), self.M, cap=cap, target=target)

    def implicit_t(self):
        L, st = N.lib(), N.stream_ptr()
        S = self._implicit_S()
        mp = rup(self.M, 64 * S)
        x = self.x_full()
        pt = self.buf("pt%d" % mp, (self.Cout, mp), torch.bfloat16)
        slabs = self.buf("slabs%d" % S, (S, self.Cout, self.ld), torch.float32)
        N.check(L.ctta_transpose_bf16(N.ptr(self.dy), 0, self.M, self.Cout, self.Cout, 0, N.ptr(pt), 0, mp, 1, st))
        N.check(L.ctta_wgrad_implicit(N.ptr(pt), self.Cout, mp, N.ptr(x), self.Cin, self.Cin, self.B, self.H, self.W, 9, self.M, S, self.K,
                                      0, N.ptr(slabs), self.Cout * self.ld, self.ld, st))
        self.scatter(slabs, S)
        return "implicit, dY^T (S=%d)" % S

    def implicit_inplace(self, cap=16, target=256):
        L, st = N.lib(), N.stream_ptr()
        S = self._implicit_S(cap, target)
        mp = rup(self.M, 64 * S)
        x = self.x_full()
        slabs = self.buf("slabs%d" % S, (S, self.Cout, self.ld), torch.float32)
        N.check(L.ctta_wgrad_implicit_inplace(N.ptr(self.dy), self.Cout, self.Cout, mp, N.ptr(x), self.Cin, self.Cin, self.B, self.H, self.W,
                                              9, self.M, S, self.K, 0, N.ptr(slabs), self.Cout * self.ld, self.ld, st))
        self.scatter(slabs, S)
        return "implicit, dY in place (S=%d)" % S + ("" if (cap, target) == (16, 256) else " <=%d, %d wg" % (cap, target))

    def implicit_direct(self):
        L, st = N.lib(), N.stream_ptr()
        x = self.x_full()
        N.check(L.ctta_wgrad_implicit_direct(N.ptr(self.dy), self.Cout, self.Cout, rup(self.M, 64), N.ptr(x), self.Cin, self.Cin, self.B,
                                             self.H, self.W, self.M, self.K, self.Cout, N.ptr(self.ro), N.ptr(self.gw), self.Cout, None,
                                             N.ptr(self.gb), st))
        return "implicit, direct (S=1)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vae_wgrad_bench needs a GPU: nothing is measured without one")
    lines = ["# weight-gradient routes at batch %d, %d x 64; %d timed replays after %d warm-ups, routes alternating; box %s, %s"
             % (a.batch, a.height, a.reps, a.warmup, socket.gethostname(), torch.cuda.get_device_name(0)),
             "%-20s %-44s %10s %10s %10s" % ("layer", "route", "median ms", "min ms", "max ms")]
    for name, cin, cout, ups in (("3x3 128->128", 128, 128, False), ("3x3 256->128", 256, 128, False),
                                 ("x2 + 3x3 256->256", 256, 256, True)):
        lay = Layer(a.batch, a.height, 64, cin, cout, ups)
        routes = [lay.copies, lay.implicit_t, lay.implicit_inplace, lay.implicit_direct]
        # more position splits: the 64 x 64 tiles of a 128-wide layer are only 4 workgroups per split.  (cap, workgroups aimed at)
        for cap, target in ((64, 256), (64, 512), (128, 1024)):
            f = functools.partial(lay.implicit_inplace, cap, target)
            f.__name__ = "implicit_inplace_%d_%d" % (cap, target)
            routes.insert(-1, f)
        ref = None
        for r in routes:      # the routes agree before they are timed
            lay.gw.zero_()
            r()
            torch.cuda.synchronize()
            got = lay.gw.clone()
            if ref is None:
                ref = got
            err = float((got - ref).abs().max() / ref.abs().max())
            assert err < 1e-3, (name, r.__name__, err)
        times = {r.__name__: [] for r in routes}
        labels = {}
        for i in range(a.warmup + a.reps):
            for r in routes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                labels[r.__name__] = r()
                e1.record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    times[r.__name__].append(e0.elapsed_time(e1))
        for r in routes:
            t = sorted(times[r.__name__])
            lines.append("%-20s %-44s %10.3f %10.3f %10.3f" % (name, labels[r.__name__], t[len(t) // 2], t[0], t[-1]))
        del lay
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
