"""Float64 references, input families, per-element bounds, column-sum emulations, the case table and a launch mirror for the
weight-gradient kernels: csrc/wgrad_gemm.hip (wgrad_implicit_kernel, wgrad_implicit_w64_kernel, wgrad_tn_kernel,
wgrad_rowsum_kernel), the ctta_im2col_t + conv_gemm route and the scatter step of csrc/backward.hip.  No GPU call at import:
test_wgrad_ref_cpu.py checks this module on the CPU, test_wgrad_forms_gpu.py uses it against the kernels.

Layouts are the kernels': x is NHWC (B, H, W, C) BEFORE an x2 upsample, dy is (M, N) with M = B * ho * wo, a weight row is
(cin, kh, kw)-ordered: dW is (N, K), K = C * taps, column c * taps + t.  A linear layer is the 1x1 case B = 1, H = rows, W = 1.

Bound, per element:   |got - ref| <= 2^-24 (L A + |ref|)
  A    the same sum over |dY| |X| (over |dY| for the column sums),
  L    the number of fp32 roundings on the longest path to the element, as the kernel is written:
         products     ceil(seg / 8) + 8 + S   (+ 1 direct, + conv_gemm's own split count on the im2col^T route) -- one
                      16x16x32 MFMA read as four chained 8-term stages, the most pessimistic reading of the instruction;
         column sums  counted from the emulated order (sums_L_*), the kernel's sums are asserted BIT FOR BIT against the
                      emulation and the emulation against float64.
  The final |ref| term is the rounding of the stored result.  bf16 x bf16 products are exact in fp32.
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn.functional as F

from consistencytta_amd import _native as N
from consistencytta_amd import spec

EPS24 = 2.0 ** -24
ROUTES = ("tn", "tn_direct", "implicit_inplace", "implicit_direct", "implicit_dyt", "im2col_t")
POLICIES = {"unet": (256, 16, 1, 0), "vae": (512, 128, 0, 1), "own": (4096, 4, 1, 1)}
FAMILIES = ("uniform", "offset", "impulse")          # + "spread" on the row-sum cases (make_inputs)


def rup(a, b):
    return (a + b - 1) // b * b


def det(name, shape, seed=0):
    return torch.from_numpy(spec.det_uniform(name, tuple(shape), seed))


def bf16_round(x):
    return x.to(torch.bfloat16).to(torch.float32)


# ------------------------------------------------------------------------------------------------ geometry
def out_hw(c):
    hi, wi = (2 * c["H"], 2 * c["W"]) if c["ups"] else (c["H"], c["W"])
    return hi, wi, (hi + 2 * c["pad"] - c["kh"]) // c["stride"] + 1, (wi + 2 * c["pad"] - c["kw"]) // c["stride"] + 1


def positions(c):
    _, _, ho, wo = out_hw(c)
    return c["B"] * ho * wo


def geom_fields(c):
    """ctta_wgrad_geom as engine_backward.h's wgrad_geom fills it."""
    hi, wi, ho, wo = out_hw(c)
    return dict(kh=c["kh"], kw=c["kw"], c=c["C"], batch=c["B"], hi=hi, wi=wi, upsample=int(c["ups"]), ho=ho, wo=wo,
                stride=c["stride"], pad=c["pad"], n=c["N"], nb=c["nb"], direct_ok=c.get("direct_ok", 0),
                run_async=c.get("run_async", 0), keeps_dy=c.get("keeps_dy", 0))


# ------------------------------------------------------------------------------------------------ references
def unfold64(x, c):
    """Q (M, K) float64: Q[m][ci * taps + t] = X[pixel(m, tap t)][ci], zero outside the image."""
    xn = x.double().permute(0, 3, 1, 2)
    if c["ups"]:
        xn = xn.repeat_interleave(2, 2).repeat_interleave(2, 3)
    q = F.unfold(xn, (c["kh"], c["kw"]), padding=c["pad"], stride=c["stride"])          # (B, K, ho * wo)
    return q.permute(0, 2, 1).reshape(-1, q.shape[1]).contiguous()


def split_refs(x, dy, c, S, seg):
    """Per split s (positions [s seg, (s + 1) seg) below M): dw (S, N, K), db (S, N), ps (S, B, N) and their absolute sums
    adw, adb, aps, all float64.  The layer's gradient is the sum over s."""
    q, d = unfold64(x, c), dy.double()
    M, B = q.shape[0], c["B"]
    hw = M // B
    out = {k: [] for k in ("dw", "adw", "db", "adb", "ps", "aps")}
    for s in range(S):
        lo, hi = min(s * seg, M), min((s + 1) * seg, M)
        qs, ds = q[lo:hi], d[lo:hi]
        out["dw"].append(ds.t() @ qs)
        out["adw"].append(ds.abs().t() @ qs.abs())
        out["db"].append(ds.sum(0))
        out["adb"].append(ds.abs().sum(0))
        ind = torch.zeros(hi - lo, B, dtype=torch.float64)
        if hi > lo:
            ind[torch.arange(hi - lo), torch.arange(lo, hi) // hw] = 1.0
        out["ps"].append(ind.t() @ ds)
        out["aps"].append(ind.t() @ ds.abs())
    return {k: torch.stack(v) for k, v in out.items()}


def autograd_refs(x, dy, c):
    """dW, db, ps from torch.autograd in float64 (what split_refs must sum to), and the same on the absolute values."""
    res = []
    for xx, dd in ((x.double(), dy.double()), (x.double().abs(), dy.double().abs())):
        xn = xx.permute(0, 3, 1, 2)
        if c["ups"]:
            xn = F.interpolate(xn, scale_factor=2.0, mode="nearest")
        w = torch.zeros(c["N"], c["C"], c["kh"], c["kw"], dtype=torch.float64, requires_grad=True)
        b = torch.zeros(c["N"], dtype=torch.float64, requires_grad=True)
        y = F.conv2d(xn, w, b, stride=c["stride"], padding=c["pad"])
        g = dd.view(c["B"], y.shape[2], y.shape[3], c["N"]).permute(0, 3, 1, 2)
        y.backward(g)
        res += [w.grad.reshape(c["N"], -1), b.grad, g.sum(dim=(2, 3))]
    return res


def bound(L, A, ref):
    return EPS24 * (L * A + ref.abs())


def worst_ratio(err, bnd):
    """max err / bound; an element with bound 0 must have error 0 (inf otherwise)."""
    err, bnd = err.double().reshape(-1), bnd.double().reshape(-1)
    if err.numel() == 0:
        return 0.0
    r = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    r = torch.where(torch.isfinite(err), r, torch.full_like(err, math.inf))
    return float(r.max())


def L_mfma(seg, S, direct=False, conv_splits=0):
    return -(-seg // 8) + 8 + S + (1 if direct else 0) + conv_splits


# ------------------------------------------------------------------------------------------------ inputs
def impulse_sites(c, S, seg):
    """(b, h, w) of the impulses of a 3x3 stride-1 case, one per channel: the four corners of image 0, the last pixel of
    image 0 and the first of image 1, positions 63 and 64, both sides of the first split boundary inside M."""
    B, H, W = c["B"], c["H"], c["W"]
    flat = [0, W - 1, (H - 1) * W, H * W - 1]
    if B > 1:
        flat += [H * W - 1, H * W]
    M = B * H * W
    flat += [m for m in (63, 64) if m < M]
    if S > 1 and seg < M:
        flat += [seg - 1, seg]
    return [(m // (H * W), (m % (H * W)) // W, m % W) for m in flat]


def impulse_channel(i, C):
    return C - 1 - 3 * i          # from the last (ragged) 8-block downwards, one channel per site


def make_inputs(c, family, S=1, seg=0):
    """x (B, H, W, C) and dy (M, N), fp32 tensors of bf16-representable values."""
    B, H, W, C, Nn = c["B"], c["H"], c["W"], c["C"], c["N"]
    M = positions(c)
    tag = "wg.%s" % c["id"]
    if family == "uniform":
        return bf16_round(det(tag + ".x", (B, H, W, C), 1)), bf16_round(det(tag + ".dy", (M, Nn), 4))
    if family == "offset":
        return bf16_round(2.0 + det(tag + ".x", (B, H, W, C), 1)), bf16_round(3.0 + 0.5 * det(tag + ".dy", (M, Nn), 4))
    if family == "spread":
        # dY with magnitudes 1, 2^-9 and 2^-18 side by side: already the sum of one 8-position block rounds in fp32, so the
        # ORDER inside a block shows in the bits (eight zero-mean bf16 values of one magnitude add exactly in any order)
        m, n = torch.arange(M).view(M, 1), torch.arange(Nn).view(1, Nn)
        dy = bf16_round(det(tag + ".dy", (M, Nn), 4)) * torch.pow(2.0, -9.0 * ((m + n) % 3).float())
        assert torch.equal(dy, bf16_round(dy))
        return bf16_round(det(tag + ".x", (B, H, W, C), 1)), dy
    assert family == "impulse" and c["kh"] == 3 and c["stride"] == 1 and not c["ups"]
    x = torch.zeros(B, H, W, C)
    for i, (b, h, w) in enumerate(impulse_sites(c, S, seg)):
        x[b, h, w, impulse_channel(i, C)] = 1.0
    m, n = torch.arange(M).view(M, 1), torch.arange(Nn).view(1, Nn)
    dy = (((7 * m + 3 * n) % 251) - 125).float()
    assert torch.equal(dy, bf16_round(dy))
    return x, dy


# ------------------------------------------------------------------------------------------------ column sums, emulated
def _seq32(a):
    """Sequential fp32 sum over axis 0, starting from 0.f."""
    t = np.zeros(a.shape[1:], np.float32)
    for r in range(a.shape[0]):
        t = t + a[r]
    return t


def _padded(dy, mp):
    d = np.zeros((mp, dy.shape[1]), np.float32)
    d[: dy.shape[0]] = dy.numpy().astype(np.float32)
    return d


def emu_sums_implicit(dy, M, mp, S, HW, sample_cols, batch):
    """park + fold_sums of the in-place 3x3 kernels (both copies): a thread adds rows p and p + 32 of every 64-row chunk to
    its running sums (32 row phases p), a fold adds the 32 phases in order; with per-sample columns a fold happens at every
    sample boundary and the bias column is the running total of the folds.  -> bias (S, N), ps (S, batch, N) fp32
    (samples >= sample_cols stay 0: the kernel has no column for them)."""
    d, seg, Nn = _padded(dy, mp), mp // S, dy.shape[1]
    bias, ps = np.zeros((S, Nn), np.float32), np.zeros((S, batch, Nn), np.float32)
    for s in range(S):
        bsum, tot, acc = np.zeros((32, Nn), np.float32), np.zeros(Nn, np.float32), -1

        def fold(sample):
            nonlocal bsum, tot
            t = _seq32(bsum)
            bsum = np.zeros((32, Nn), np.float32)
            tot = tot + t
            if 0 <= sample < sample_cols:
                ps[s, sample] = t

        for m0 in range(s * seg, min((s + 1) * seg, mp), 64):
            if sample_cols > 0 and m0 < M:
                b = m0 // HW
                if acc >= 0 and b != acc:
                    fold(acc)
                acc = b
            bsum = bsum + d[m0:m0 + 32]
            bsum = bsum + d[m0 + 32:m0 + 64]
        fold(acc)
        bias[s] = tot
    return torch.from_numpy(bias), torch.from_numpy(ps)


def sums_L_implicit(seg, S, HW, sample_cols):
    folds = (-(-seg // HW) + 1) if sample_cols > 0 else 1
    return 2 * (seg // 64) + 32 + folds + S


def emu_sums_tn(dy, M, mp, S):
    """add_bias + the 16-phase fold of wgrad_tn_kernel: a thread adds rows p, p + 16, p + 32, p + 48 of every chunk (16 row
    phases p), the fold adds the phases in order.  -> (S, N) fp32."""
    d, seg, Nn = _padded(dy, mp), mp // S, dy.shape[1]
    out = np.zeros((S, Nn), np.float32)
    for s in range(S):
        bsum = np.zeros((16, Nn), np.float32)
        for m0 in range(s * seg, (s + 1) * seg, 64):
            for i in range(4):
                bsum = bsum + d[m0 + 16 * i:m0 + 16 * i + 16]
        out[s] = _seq32(bsum)
    return torch.from_numpy(out)


def sums_L_tn(seg, S):
    return 4 * (seg // 64) + 16 + S


def emu_sums_rowsum(dy, M, mp, S, hw, nb, batch):
    """wgrad_rowsum_kernel: per (channel, split, sample part) lane l adds the pairwise-tree sums of its 8-position blocks at
    a + 8 l + 512 k, then the ragged tail one by one, then the xor butterfly 32 .. 1; the bias column is the running total of
    the parts (the positions behind the last per-sample column included).  -> bias (S, N), ps (S, batch, N) fp32."""
    d, seg, Nn = _padded(dy, mp).T.copy(), mp // S, dy.shape[1]           # (N, mp)
    bias, ps = np.zeros((S, Nn), np.float32), np.zeros((S, batch, Nn), np.float32)
    lanes = np.arange(64)
    for s in range(S):
        lo, hi = s * seg, min(min((s + 1) * seg, mp), M)
        parts = [(b, max(lo, b * hw), min(hi, (b + 1) * hw)) for b in range(nb)] + [(-1, max(lo, nb * hw), hi)] if nb > 0 else [(-1, lo, hi)]
        total = np.zeros(Nn, np.float32)
        for b, a, e in parts:
            v = np.zeros((64, Nn), np.float32)
            for l in range(64):
                m = a + 8 * l
                sm = np.zeros(Nn, np.float32)
                while m + 8 <= e:
                    f = d[:, m:m + 8]
                    sm = sm + (((f[:, 0] + f[:, 1]) + (f[:, 2] + f[:, 3])) + ((f[:, 4] + f[:, 5]) + (f[:, 6] + f[:, 7])))
                    m += 512
                for t in range(m, min(e, m + 8)):
                    sm = sm + d[:, t]
                v[l] = sm
            for o in (32, 16, 8, 4, 2, 1):
                v = v + v[lanes ^ o]
            total = total + v[0]
            if b >= 0:
                ps[s, b] = v[0]
        bias[s] = total
    return torch.from_numpy(bias), torch.from_numpy(ps)


def sums_L_rowsum(seg, S, nb):
    return -(-seg // 512) + 3 + 7 + 6 + nb + 1 + S


def emu_products(x, dy, c, S, seg):
    """fp32 emulation of the split-M product: inside a split, blocks of 8 positions are summed in fp32 one term at a time and
    the block sums are chained in fp32; the splits are then added in order.  -> (N, K) fp32 as float64."""
    q, d = unfold64(x, c).numpy().astype(np.float32), dy.numpy().astype(np.float32)
    M, K = q.shape
    mp = S * seg
    qp, dp = np.zeros((mp, K), np.float32), np.zeros((mp, d.shape[1]), np.float32)
    qp[:M], dp[:M] = q, d
    tot = np.zeros((d.shape[1], K), np.float32)
    for s in range(S):
        lo, hi = s * seg, min((s + 1) * seg, rup(M, 8))
        acc = np.zeros_like(tot)
        if hi > lo:
            qb, db = qp[lo:hi].reshape(-1, 8, K), dp[lo:hi].reshape(-1, 8, d.shape[1])
            blk = np.zeros((qb.shape[0],) + tot.shape, np.float32)
            for j in range(8):                                   # one term at a time, every block at once
                blk = blk + db[:, j, :, None] * qb[:, j, None, :]
            acc = np.add.accumulate(blk, axis=0, dtype=np.float32)[-1]          # the chain: one block sum at a time
        tot = tot + acc
    return torch.from_numpy(tot.astype(np.float64))


# ------------------------------------------------------------------------------------------------ dispatch predicates
def implicit_supported(taps, c, h, w, x_ld, n):
    """ctta_wgrad_implicit_supported"""
    if c < 32 or c % 8 or x_ld % 8 or n < 8:
        return False
    if taps == 1:
        return True
    if taps != 9 or w < 2 or w > 64 or (w & (w - 1)):
        return False
    return (h * w) % 64 == 0


def implicit_kernel(taps, w, nat):
    """The kernel wgrad_implicit_launch picks."""
    if taps == 9 and w == 64:
        return "w64<nat>" if nat else "w64<dyt>"
    if taps == 9:
        return "generic<9,nat>" if nat else "generic<9,dyt>"
    return "generic<1>"


def _splits_for(tiles, M, target, cap, min_m):
    S = 1
    while tiles * S < target and S < cap and M // (2 * S) >= min_m:
        S *= 2
    return S


def _tiles(a, ta, b, tb):
    return ((a + ta - 1) // ta) * ((b + tb - 1) // tb)


def plan_py(g, pol):
    """ctta_wgrad_plan's rules: route name, splits, mp, seg, rows, ld, sums_apart, upsample_copy."""
    target, cap, pdirect, ucopy = pol
    taps, C, Nn, nb = g["kh"] * g["kw"], g["c"], g["n"], g["nb"]
    M = g["batch"] * g["ho"] * g["wo"]
    rows = taps * C + 1 + nb
    direct = bool(pdirect and g["direct_ok"] and nb == 0)
    up = 0
    if taps == 1 and not g["upsample"] and g["stride"] == 1 and g["pad"] == 0 and nb == 0 and C % 8 == 0 and Nn % 8 == 0:
        S = _splits_for(_tiles(Nn, 128, C, 128), M, 256, 32, 128)
        route = "tn_direct" if S == 1 and direct else "tn"
    elif ((not g["upsample"] or ucopy) and g["stride"] == 1 and g["ho"] == g["hi"] and g["wo"] == g["wi"] and taps == 9 and
          g["kh"] == 3 and g["pad"] == 1 and implicit_supported(9, C, g["hi"], g["wi"], C, Nn)):
        S = _splits_for(_tiles(Nn, 64, C, 64), M, target, cap, 256)
        inplace = Nn % 8 == 0 and (nb == 0 or (g["ho"] * g["wo"]) % 64 == 0) and (not g["run_async"] or g["keeps_dy"])
        route = "implicit_dyt" if not inplace else "implicit_direct" if S == 1 and direct else "implicit_inplace"
        up = 1 if g["upsample"] else 0
    else:
        S = _splits_for(_tiles(rows, 128, Nn, 128), M, 256, 16, 256)
        route = "im2col_t"
    mp = rup(M, 64 * S)
    sums_apart = int(route == "im2col_t" and (nb == 0 or (g["ho"] * g["wo"]) % 8 == 0) and mp % (8 * S) == 0)
    return dict(route=route, splits=S, mp=mp, seg=mp // S, rows=rows, ld=rup(rows, 4), sums_apart=sums_apart, upsample_copy=up)


def plan_real(lib, g, pol):
    out = N.WgradPlanInfo()
    st = lib.ctta_wgrad_plan(ctypes.byref(N.WgradGeom(**g)), ctypes.byref(N.WgradPolicy(*pol)), ctypes.byref(out))
    assert st == 0, lib.ctta_last_error().decode()
    return out


def gemm_desc(pt, q, slabs, Nn, n_cols, S, seg, mp, ld):
    """The conv_gemm descriptor of the im2col^T route (wgrad_launch): slabs[s][n][r] = sum_m dY^T[n][m] Q[r][m] over split s."""
    d = N.ConvDesc()
    d.kh = d.kw = d.stride_h = d.stride_w = d.dil_h = d.dil_w = 1
    d.alpha = 1.0
    d.x0, d.c0, d.x_stride = pt, seg, mp
    d.batch, d.hi, d.wi, d.ho, d.wo = 1, Nn, 1, Nn, 1
    d.w, d.k_pad, d.n = q, mp, n_cols
    d.out, d.ldc, d.out_f32 = slabs, ld, 1
    d.groups, d.x_group_stride, d.w_group_stride, d.out_group_stride = S, seg, seg, Nn * ld
    return d


# The environment ctta_conv_plan is asked under: assumed to be what ctta_conv_gemm plans with on one MI355X with its default
# options (256 CUs, split-K and stream-K on, the default 192 MB workspace).  A launch that planned MORE splits than this
# reports would make the L term too small: the bound then fails safe (a test goes red, nothing passes wrongly).
PLAN_ENV = dict(cu_count=256, xcd=1, splitk=1, streamk=1, streamk_grid=0, suppress_splitk=0, stamps_bound=0,
                workspace_bytes=192 << 20, workspace_header_zeroed=1)


def gemm_splits(lib, Nn, n_cols, S, seg, mp, ld):
    """The split count ctta_conv_plan reports for that descriptor (pointers are only looked at for NULL)."""
    info = N.ConvPlanInfo()
    d = gemm_desc(0x1000, 0x1000, 0x1000, Nn, n_cols, S, seg, mp, ld)
    st = lib.ctta_conv_plan(ctypes.byref(d), ctypes.byref(N.ConvPlanEnv(**PLAN_ENV)), ctypes.byref(info))
    assert st == 0, lib.ctta_last_error().decode()
    return max(1, info.splits)


# ------------------------------------------------------------------------------------------------ the case table
def _case(id, kind, B, C, H, W, Nn, nb=0, S=1, bias=True, x_ld=None, ldy=None, kh=3, kw=3, stride=1, pad=1, ups=False,
          policy=None, families=("uniform", "offset"), **extra):
    c = dict(id=id, kind=kind, B=B, C=C, H=H, W=W, N=Nn, nb=nb, S=S, bias=bias, x_ld=x_ld or C, ldy=ldy or Nn, kh=kh, kw=kw,
             stride=stride, pad=pad, ups=ups, policy=policy, families=tuple(families))
    c.update(extra)
    return c


def _i3_cases():
    out = []
    # widths: one chunk is one image (H W = 64), and the patch's outer rows belong to the neighbouring chunk (H W = 128);
    # B = 2, one split, per-sample columns: a sample boundary between chunks folds the sums
    for W in (2, 4, 8, 16, 32, 64):
        for HW in (64, 128):
            out.append(_case("i3-W%d-HW%d" % (W, HW), "i3", 2, 32, HW // W, W, 8, nb=2, S=1, families=FAMILIES))
    for W in (2, 4, 16, 32):    # a split boundary inside an image at the other widths too (W = 8 and 64 follow): seg = 64 of H W = 128
        out.append(_case("i3-W%d-S4" % W, "i3", 2, 32, 128 // W, W, 8, S=4, families=FAMILIES))
    for W in (16, 32):          # the U-Net's and the VAE's plain convolutions at these widths: no per-sample columns
        out.append(_case("i3-W%d-nb0" % W, "i3", 2, 32, 128 // W, W, 8, S=2, families=FAMILIES))
    # the same edge classes on the generic kernel (W = 8) and on its width-64 copy
    for W in (8, 64):
        H = 128 // W
        for C, Nn in ((32, 8), (40, 24), (72, 72)):
            out.append(_case("i3-W%d-C%d-N%d" % (W, C, Nn), "i3", 2, C, H, W, Nn, S=2, families=FAMILIES))
        for S in (1, 2, 3, 4, 8):          # M = 256: S = 4 -> seg 64, a boundary inside an image; S = 3, 8 -> empty splits
            out.append(_case("i3-W%d-S%d" % (W, S), "i3", 2, 32, H, W, 8, S=S, families=FAMILIES))
        out.append(_case("i3-W%d-nbB" % W, "i3", 2, 32, H, W, 24, nb=2, S=2, families=FAMILIES))
        out.append(_case("i3-W%d-nb1of3" % W, "i3", 3, 32, H, W, 24, nb=1, S=2, families=FAMILIES))
        out.append(_case("i3-W%d-nb0-bias" % W, "i3", 2, 32, H, W, 24, nb=0, S=2, families=FAMILIES))
        out.append(_case("i3-W%d-nobias" % W, "i3", 2, 32, H, W, 24, nb=0, S=2, bias=False, families=FAMILIES))
        out.append(_case("i3-W%d-strided" % W, "i3", 2, 40, H, W, 24, nb=2, S=2, x_ld=56, ldy=40, families=FAMILIES))
    return out


def _lin(id, kind, M, C, Nn, **kw):
    return _case(id, kind, 1, C, M, 1, Nn, kh=1, kw=1, pad=0, **kw)


def _tn_cases():
    return [
        _lin("tn-M1", "tn", 1, 8, 8),
        _lin("tn-M63", "tn", 63, 128, 136),
        _lin("tn-M64", "tn", 64, 136, 128),
        _lin("tn-M65", "tn", 65, 264, 8, S=2),
        _lin("tn-M200-strided", "tn", 200, 8, 264, x_ld=16, ldy=272),
        _lin("tn-M200-nobias", "tn", 200, 128, 128, S=2, bias=False),
        _lin("tn-M200-264", "tn", 200, 264, 264, S=3, x_ld=272, ldy=264),
        _lin("tn-M1088-S8", "tn", 1088, 128, 128, S=8),          # the plan's own S, mp = 1536: two empty splits, one ragged
    ]


def _i1_cases():
    return [_lin("i1-M77", "i1", 77, 32, 24, S=2), _lin("i1-M200-C264", "i1", 200, 264, 40, S=1),
            _lin("i1-M300-nobias", "i1", 300, 40, 72, S=2, bias=False, x_ld=48)]


def _rowsum_cases():
    out = []
    for M, B, nb, S in ((77, 1, 0, 1), (77, 1, 0, 2), (512, 2, 0, 1), (512, 2, 2, 2), (520, 5, 5, 1), (520, 5, 0, 2),
                        (520, 5, 5, 2), (512, 4, 2, 2)):
        out.append(_case("rs-M%d-B%d-nb%d-S%d" % (M, B, nb, S), "rowsum", B, 8, M // B, 1, 24, nb=nb, S=S, kh=1, kw=1, pad=0,
                         families=("uniform", "offset", "spread")))
    return out


def _mirror_cases():
    u, v, o = "unet", "vae", "own"
    return [
        # im2col^T route
        _case("m-stride2", "mirror", 2, 32, 8, 8, 24, stride=2, policy=u),
        _case("m-stride2-vae", "mirror", 2, 32, 8, 8, 24, stride=2, policy=v),
        _case("m-ups-nocopy", "mirror", 2, 32, 4, 4, 24, ups=True, policy=u),
        _case("m-convin-c8", "mirror", 2, 8, 8, 8, 32, policy=u),
        _case("m-stride2-nb-apart", "mirror", 2, 32, 8, 8, 24, nb=2, stride=2, policy=u),        # ho wo = 16: sums apart
        _case("m-stride2-nb-rows", "mirror", 2, 32, 6, 6, 24, nb=2, stride=2, policy=u),         # ho wo = 9: indicator rows
        _case("m-stride2-S2", "mirror", 9, 32, 16, 16, 24, stride=2, policy=o),                  # M = 576: two splits
        # the widths the recorded real layers take on this route: every column at the border with the per-sample columns riding
        # along (wi = 2: sums apart; wi = 3: indicator rows), conv_in at wi = 16, the x2 upsample at wi = 6, 32, 64, 128
        _case("m-res-w2-nb", "mirror", 2, 32, 4, 2, 24, nb=2, policy=u),
        _case("m-res-w3-nb", "mirror", 2, 32, 4, 3, 24, nb=2, policy=u),
        _case("m-convin-c8-w16", "mirror", 2, 8, 4, 16, 32, policy=u),
        _case("m-stride2-w16", "mirror", 2, 32, 16, 16, 24, stride=2, policy=u),
        _case("m-ups-w6", "mirror", 2, 32, 3, 3, 24, ups=True, policy=u),
        _case("m-ups-w6-vae", "mirror", 2, 32, 3, 3, 24, ups=True, policy=v),
        _case("m-ups-w32", "mirror", 1, 32, 2, 16, 24, ups=True, policy=u),
        _case("m-ups-w64", "mirror", 1, 32, 1, 32, 24, ups=True, policy=u),
        _case("m-ups-w128", "mirror", 1, 32, 1, 64, 24, ups=True, policy=u),
        _case("m-ups-w128-vae", "mirror", 1, 32, 1, 64, 24, ups=True, policy=v),
        # implicit routes
        _case("m-ups-copy", "mirror", 2, 32, 4, 4, 24, ups=True, policy=v),
        _case("m-i3-inplace-empty-split", "mirror", 33, 32, 8, 8, 8, policy=u, direct_ok=1),      # M = 33 * 64: S = 8, mp = 40 * 64
        _case("m-i3-inplace-vae", "mirror", 2, 32, 8, 8, 24, policy=v, direct_ok=1),
        _case("m-i3-inplace-nb", "mirror", 2, 40, 8, 8, 24, nb=2, policy=u),
        _case("m-i3-direct", "mirror", 2, 40, 8, 8, 24, policy=u, direct_ok=1),
        _case("m-i3-direct-own", "mirror", 2, 32, 2, 64, 24, policy=o, direct_ok=1),
        _case("m-i3-dyt", "mirror", 2, 40, 8, 8, 24, nb=2, policy=u, run_async=1, keeps_dy=0),
        _case("m-i3-w64-S2", "mirror", 8, 32, 1, 64, 8, policy=o),                               # M = 512: two splits
        # linears
        _lin("m-tn-plan-M1088", "mirror", 1088, 128, 128, policy=u, direct_ok=1),                # S = 8, mp = 1536, seg = 192
        _lin("m-tn-vae", "mirror", 300, 136, 40, policy=v, direct_ok=1),
        _lin("m-tn-direct", "mirror", 200, 128, 136, policy=u, direct_ok=1),
        _lin("m-tn-direct-colmap", "mirror", 77, 40, 24, policy=u, direct_ok=1, colmap=True),
    ]


CASES = _i3_cases() + _tn_cases() + _i1_cases() + _rowsum_cases() + _mirror_cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def case_params():
    """(case, family) pairs of the numeric tests."""
    return [(c, f) for c in CASES for f in c["families"]]


def forced_plan(c):
    """splits / mp / seg / ld of a forced-route case."""
    M, S = positions(c), c["S"]
    mult = 8 if c["kind"] == "rowsum" else 64
    mp = rup(M, mult * S)
    K = c["kh"] * c["kw"] * c["C"]
    return dict(splits=S, mp=mp, seg=mp // S, rows=K + 1 + c["nb"], ld=rup(K + 1 + c["nb"], 4))


def classes(c, plan=None):
    """The geometry classes a case stands for.  `plan`: the plan of a mirror case (plan_py or the real one, as a dict)."""
    kind = c["kind"]
    p = plan if kind == "mirror" else forced_plan(c)
    M, S, seg = positions(c), p["splits"], p["seg"]
    out = set()
    empty = any(s * seg >= M for s in range(S))
    if kind == "i3":
        hw = c["H"] * c["W"]
        k = implicit_kernel(9, c["W"], True).split("<")[0]
        out |= {"i3:%s:C%d" % (k, c["C"]), "i3:%s:N%d" % (k, c["N"]), "i3:%s:S%d" % (k, S)}
        if S == 1 and c["nb"] == c["B"]:
            out.add("i3:W%d:HW%d" % (c["W"], hw))
        if seg < hw and S > 1:
            out |= {"i3:%s:split-in-image" % k, "i3:W%d:split-in-image" % c["W"]}
        if empty:
            out.add("i3:%s:empty-split" % k)
        if not c["bias"]:
            out.add("i3:%s:bias_col=-1" % k)
        elif c["nb"] == 0:
            out.add("i3:%s:nb=0+bias" % k)
        elif c["nb"] == c["B"]:
            out.add("i3:%s:nb=B" % k)
        else:
            out.add("i3:%s:0<nb<B" % k)
        if c["x_ld"] > c["C"]:
            out.add("i3:%s:x_ld>c" % k)
        if c["ldy"] > c["N"]:
            out.add("i3:%s:ldy>n" % k)
    elif kind == "tn":
        out |= {"tn:M%d" % M, "tn:C%d" % c["C"], "tn:N%d" % c["N"], "tn:bias_col=%s" % ("C" if c["bias"] else "-1")}
        if c["x_ld"] > c["C"]:
            out.add("tn:ldx>c")
        if c["ldy"] > c["N"]:
            out.add("tn:ldy>n")
        if empty:
            out.add("tn:empty-split")
    elif kind == "i1":
        out |= {"i1:C%d" % c["C"]}
        if M % 64:
            out.add("i1:ragged-M")
        if c["N"] % 64:
            out.add("i1:ragged-N")
    elif kind == "rowsum":
        out |= {"rs:M%d" % M, "rs:S%d" % S, "rs:nb=%s" % ("0" if c["nb"] == 0 else "B" if c["nb"] == c["B"] else "part")}
    else:
        r = p["route"]
        out.add("m:%s:%s" % (c["policy"], r))
        if r == "im2col_t":
            if c["stride"] == 2:
                out.add("m:im2col:stride2")
            if c["ups"]:
                out.add("m:im2col:upsample")
            if c["C"] == 8:
                out.add("m:im2col:conv_in8")
            if c["nb"] > 0:
                out.add("m:im2col:nb:sums_apart=%d" % p["sums_apart"])
        if c["ups"]:
            out.add("m:upsample_copy=%d" % p["upsample_copy"])
        if empty:
            out.add("m:%s:empty-split" % ("tn" if r.startswith("tn") else "i3" if r.startswith("implicit") else r))
    return out


def _required():
    req = set()
    for W in (2, 4, 8, 16, 32, 64):
        req |= {"i3:W%d:HW64" % W, "i3:W%d:HW128" % W, "i3:W%d:split-in-image" % W}
    for k in ("generic", "w64"):
        req |= {"i3:%s:C%d" % (k, v) for v in (32, 40, 72)} | {"i3:%s:N%d" % (k, v) for v in (8, 24, 72)}
        req |= {"i3:%s:S%d" % (k, v) for v in (1, 2, 3, 4, 8)}
        req |= {"i3:%s:%s" % (k, v) for v in ("split-in-image", "empty-split", "nb=B", "0<nb<B", "nb=0+bias", "bias_col=-1",
                                              "x_ld>c", "ldy>n")}
    req |= {"tn:M%d" % v for v in (1, 63, 64, 65, 200, 1088)} | {"tn:C%d" % v for v in (8, 128, 136, 264)}
    req |= {"tn:N%d" % v for v in (8, 128, 136, 264)} | {"tn:ldx>c", "tn:ldy>n", "tn:bias_col=C", "tn:bias_col=-1", "tn:empty-split"}
    req |= {"i1:ragged-M", "i1:ragged-N", "i1:C32", "i1:C264"}
    req |= {"rs:M77", "rs:M512", "rs:M520", "rs:nb=0", "rs:nb=B", "rs:S1", "rs:S2"}
    req |= {"m:im2col:stride2", "m:im2col:upsample", "m:im2col:conv_in8", "m:im2col:nb:sums_apart=0", "m:im2col:nb:sums_apart=1",
            "m:upsample_copy=0", "m:upsample_copy=1", "m:i3:empty-split", "m:tn:empty-split"}
    return req


REQUIRED_CLASSES = _required()


# ------------------------------------------------------------------------------------------------ device helpers and the mirror
def dev_matrix(t, ld, dev, fill=float("nan")):
    """(rows, cols) fp32 -> bf16 (rows, ld) on the device, the columns [cols, ld) poisoned."""
    rows, cols = t.shape
    out = torch.full((rows, ld), fill, dtype=torch.bfloat16, device=dev)
    out[:, :cols] = t.to(torch.bfloat16).to(dev)
    return out


def pack_map(c, drop_row=None, zero=True):
    """The pack map of one layer: identity columns (or, `colmap`, the first and last column dropped), rows in order,
    `drop_row` a padding row (-1).  -> dict(ro, co, kd, bidx) on the CPU."""
    K = c["kh"] * c["kw"] * c["C"]
    co, kd = None, K
    if c.get("colmap"):
        co = torch.arange(K, dtype=torch.int32) - 1
        co[0], co[K - 1] = -1, -1
        kd = K - 2
    ro = torch.arange(c["N"], dtype=torch.int32) * kd
    bidx = torch.arange(c["N"], dtype=torch.int32)
    if drop_row is not None:
        ro[drop_row], bidx[drop_row] = -1, -1
    return dict(ro=ro, co=co, kd=kd, bidx=bidx)


def run_layer(lib, c, pol, x, dy, pm, dev):
    """wgrad_launch + scatter_wgrad of engine_backward.h: plan the layer, allocate what the plan says, launch the plan's route
    with the plan's splits / mp / seg / ld, scatter.  x (B H W, C) and dy (M, N) bf16 on the device, dense.  The gradients
    start at zero.  -> dict(plan, gw (N, kd), gb (N), ps (nb, N), slabs or None)."""
    g = geom_fields(c)
    pl = plan_real(lib, g, pol)
    st = N.stream_ptr()
    C, Nn, B, S, mp, ld = g["c"], g["n"], g["batch"], pl.splits, pl.mp, pl.ld
    K = g["kh"] * g["kw"] * C
    M = B * g["ho"] * g["wo"]
    stride = Nn * ld
    nanb = lambda n: torch.full((n,), float("nan"), dtype=torch.bfloat16, device=dev)      # noqa: E731
    q = nanb(pl.q) if pl.q else None
    pt = nanb(pl.pt) if pl.pt else None
    xu = nanb(pl.xu) if pl.xu else None
    slabs = torch.full((pl.slabs,), float("nan"), device=dev) if pl.slabs else None
    ro, bidx = pm["ro"].to(dev), pm["bidx"].to(dev)
    co = pm["co"].to(dev) if pm["co"] is not None else None
    gw, gb = torch.zeros(Nn * pm["kd"], device=dev), torch.zeros(Nn, device=dev)
    ps = torch.zeros(max(g["nb"], 1), Nn, device=dev)
    k_ident = 0 if co is not None else K
    if pt is not None:
        N.check(lib.ctta_transpose_bf16(N.ptr(dy), 0, M, Nn, Nn, 0, N.ptr(pt), 0, mp, 1, st))
    if xu is not None:
        N.check(lib.ctta_upsample2_nearest(N.ptr(x), N.ptr(xu), B, g["hi"] // 2, g["wi"] // 2, C, st))
        x = xu
    route = ROUTES[pl.route]
    if route == "tn":
        N.check(lib.ctta_wgrad_tn(N.ptr(dy), Nn, Nn, N.ptr(x), C, C, M, mp, S, K, N.ptr(slabs), stride, ld, st))
    elif route == "tn_direct":
        N.check(lib.ctta_wgrad_tn_direct(N.ptr(dy), Nn, Nn, N.ptr(x), C, C, M, mp, k_ident if k_ident > 0 else K, Nn, N.ptr(ro),
                                         N.ptr(co), N.ptr(gw), Nn, N.ptr(bidx), N.ptr(gb), st))
    elif route == "implicit_inplace":
        N.check(lib.ctta_wgrad_implicit_inplace(N.ptr(dy), Nn, Nn, mp, N.ptr(x), C, C, B, g["hi"], g["wi"], 9, M, S, K, g["nb"],
                                                N.ptr(slabs), stride, ld, st))
    elif route == "implicit_direct":
        N.check(lib.ctta_wgrad_implicit_direct(N.ptr(dy), Nn, Nn, mp, N.ptr(x), C, C, B, g["hi"], g["wi"], M, k_ident, Nn, N.ptr(ro),
                                               N.ptr(gw), Nn, N.ptr(bidx), N.ptr(gb), st))
    elif route == "implicit_dyt":
        N.check(lib.ctta_wgrad_implicit(N.ptr(pt), Nn, mp, N.ptr(x), C, C, B, g["hi"], g["wi"], 9, M, S, K, g["nb"], N.ptr(slabs),
                                        stride, ld, st))
    else:
        N.check(lib.ctta_im2col_t(N.ptr(x), C, B, g["hi"], g["wi"], g["upsample"], g["ho"], g["wo"], g["kh"], g["kw"], g["stride"],
                                  g["pad"], g["pad"], 1, N.ptr(q), mp, g["nb"], st))
        d = gemm_desc(pt.data_ptr(), q.data_ptr(), slabs.data_ptr(), Nn, K if pl.sums_apart else pl.rows, S, pl.seg, mp, ld)
        N.check(lib.ctta_conv_gemm(ctypes.byref(d), st))
        if pl.sums_apart:
            N.check(lib.ctta_wgrad_rowsum(N.ptr(pt), Nn, mp, M, S, g["ho"] * g["wo"], g["nb"], N.ptr(slabs), stride, ld, K, st))
    if slabs is not None:          # scatter_wgrad: weight rows and the bias column in one launch, then the per-sample columns
        N.check(lib.ctta_wgrad_scatter_rows_bias(N.ptr(slabs), S, stride, ld, k_ident if k_ident > 0 else K, Nn, N.ptr(ro), N.ptr(co),
                                                 N.ptr(gw), K, Nn, N.ptr(bidx), N.ptr(gb), 1, st))
        if g["nb"] > 0:
            N.check(lib.ctta_col_scatter(N.ptr(slabs), S, stride, ld, K + 1, g["nb"], Nn, None, N.ptr(ps), Nn, 0, st))
    torch.cuda.synchronize()
    return dict(plan=pl, gw=gw.view(Nn, pm["kd"]), gb=gb, ps=ps[:g["nb"]], q=q,
                slabs=slabs.view(S, Nn, ld) if slabs is not None else None)
