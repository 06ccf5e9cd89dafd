"""Kernels that only the T5 / VAE / HiFi-GAN engines (or nobody) reach, each against a float64 reference on the CPU.

The engine tests hold whole-model outputs to 2.5e-2 .. 5e-2 relative L2; one wrong border column, a vector missed by a
grid-stride loop or an unzeroed pad lane stays far below that.  Here every element is checked:

  * outputs the kernel rounds to bf16:  |got - ref| <= 2^-8 |ref| + 1e-6 max|ref|  (one bf16 rounding is 2^-9 relative;
    the rest is fp32 accumulation slack),
  * pure moves and conversions: bit for bit.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from consistencytta_amd import _native as N  # noqa: E402
from gpu_util import DEV, bf16_round, det, sync  # noqa: E402

POISON = 776.0           # exactly representable in bf16 and fp32, outside every value a kernel here produces


def lib():
    return N.lib()


def f32(x):
    """The value a C float argument takes."""
    return float(np.float32(x))


def assert_bf16_close(got, ref, what=""):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    tol = ref.abs() * 2.0 ** -8 + 1e-6 * float(ref.abs().max())
    excess = (got - ref).abs() - tol
    assert float(excess.max()) <= 0.0, (what, "worst excess %.3e at flat index %d" % (float(excess.max()), int(excess.argmax())))


def launcher_block_cap(kernel):
    """The block cap a launcher of backward.hip passes to grid1d for `kernel` (its default when it passes none)."""
    src = open(os.path.join(N.CSRC, "backward.hip")).read()
    m = re.search(r"hipLaunchKernelGGL\(%s, dim3\(grid1d\(([^;]*?)\)\), dim3\(256\)" % kernel, src)
    assert m, kernel
    args = [a.strip() for a in m.group(1).split(",")]
    if len(args) == 3:
        assert args[1] == "256"
        return int(args[2])
    assert len(args) == 1
    d = re.search(r"static int grid1d\(long long total, int per = 256, int cap = (\d+)\)", src)
    assert d
    return int(d.group(1))


def upload_table(rows):
    """A ctypes array of job structs -> device bytes."""
    raw = ctypes.string_at(ctypes.addressof(rows), ctypes.sizeof(rows))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)


# ------------------------------------------------------------------------------------ conv_cout1_dgrad
def _cout1_case(B, H, W, C, kh, kw, ph, pw, tanh, act_slope, tag, autograd=True):
    gy = det(tag + ".gy", (B, 1, H, W), 1)
    wt = det(tag + ".w", (1, C, kh, kw), 2) * 0.5
    yt = torch.tanh(det(tag + ".yt", (B, 1, H, W), 3) * 2.0) if tanh else None
    g = gy.double()
    if tanh:
        g = g * (1.0 - yt.double() ** 2)                      # the conv sat under a tanh whose output is y_tanh
    # the same sum written out tap by tap, NHWC: dx[b][y][x][c] = sum_taps w[c][a][q] g[b][y - a + ph][x - q + pw]
    gp = F.pad(g[:, 0], (kw - 1 - pw, pw, kh - 1 - ph, ph))
    ref = torch.zeros(B, H, W, C, dtype=torch.float64)
    for a in range(kh):
        for q in range(kw):
            ref += gp[:, kh - 1 - a:kh - 1 - a + H, kw - 1 - q:kw - 1 - q + W, None] * wt[0, :, a, q].double()
    if autograd:
        # reference: float64 autograd of F.conv2d for its input (the tap sum stands in for it only at the one size
        # where the CPU convolution would need gigabytes, after agreeing with it here)
        x = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(x, wt.double(), padding=(ph, pw)).backward(g)
        auto = x.grad.permute(0, 2, 3, 1)
        assert float((auto - ref).abs().max()) <= 1e-12 * float(auto.abs().max())
        ref = auto.contiguous()
    act = None
    if act_slope is not None:
        act = bf16_round(det(tag + ".act", (B, H, W, C), 4))
        act.view(-1)[::5] = 0.0                               # exactly 0: takes the slope branch
        act.view(-1)[3::7] = -0.0
        ref = ref * torch.where(act > 0, 1.0, f32(act_slope)).double()
    wk = wt[0].permute(1, 2, 0).contiguous().to(DEV)          # [kh][kw][C] fp32
    gyd = gy.contiguous().to(DEV)
    ytd = yt.contiguous().to(DEV) if tanh else None
    actd = act.to(torch.bfloat16).to(DEV) if act is not None else None
    n = B * H * W * C
    dx = torch.full((n + 16,), POISON, dtype=torch.bfloat16, device=DEV)
    N.check(lib().ctta_conv_cout1_dgrad(N.ptr(gyd), N.ptr(ytd), N.ptr(wk), B, H, W, kh, kw, ph, pw, C, N.ptr(actd),
                                        act_slope if act_slope is not None else 0.0, N.ptr(dx), N.stream_ptr()))
    sync()
    assert bool((dx[n:].float() == POISON).all())
    assert_bf16_close(dx[:n].float().cpu().reshape(B, H, W, C), ref, tag)


@pytest.mark.parametrize("B,H,W,C", [(2, 5, 7, 16), (1, 1, 9, 8), (3, 1, 300, 32)])
@pytest.mark.parametrize("form", ["3x3", "1x7_tanh"])
def test_conv_cout1_dgrad_forms_and_borders(B, H, W, C, form):
    """The decoder's conv_out (3x3, pad 1) and the vocoder's conv_post under its tanh (1x7, pad (0, 3)) at sizes where
    every border tap clips (H = 1 clips both vertical neighbours of the 3x3)."""
    if form == "3x3":
        _cout1_case(B, H, W, C, 3, 3, 1, 1, False, None, "c1a")
    else:
        _cout1_case(B, H, W, C, 1, 7, 0, 3, True, None, "c1b")


@pytest.mark.parametrize("slope", [0.1, 0.01])
def test_conv_cout1_dgrad_act_mask(slope):
    _cout1_case(2, 5, 7, 16, 3, 3, 1, 1, False, slope, "c1c")
    _cout1_case(2, 1, 33, 8, 1, 7, 0, 3, True, slope, "c1d")


def test_conv_cout1_dgrad_second_grid_stride_trip():
    """More 8-channel vectors than cap x 256 threads: HiFi-GAN's last stage (32 channels) reaches this at batch 9."""
    cap = launcher_block_cap("conv_cout1_dgrad_kernel")
    C = 32
    W = cap * 256 // (C // 8) + 77
    assert 1 * 1 * W * (C // 8) > cap * 256
    _cout1_case(1, 1, W, C, 1, 7, 0, 3, True, None, "c1e", autograd=False)


# ------------------------------------------------------------------------------------ lrelu_bwd
def _lrelu_case(n, slope, with_res, accumulate, tag):
    alpha = 1.0 / 3.0
    g = bf16_round(det(tag + ".g", (n,), 1))
    act = bf16_round(det(tag + ".a", (n,), 2))
    act[::4] = 0.0
    act[1::8] = -0.0
    res = bf16_round(det(tag + ".r", (n,), 3)) if with_res else None
    prev = bf16_round(det(tag + ".p", (n,), 4))               # what `out` holds before the call
    ref = f32(alpha) * g.double() * torch.where(act > 0, 1.0, f32(slope)).double()
    if with_res:
        ref = ref + res.double()
    if accumulate:
        ref = ref + prev.double()
    out = torch.full((n + 8,), POISON, dtype=torch.bfloat16, device=DEV)
    out[:n] = prev.to(torch.bfloat16).to(DEV)
    gd, ad = g.to(torch.bfloat16).to(DEV), act.to(torch.bfloat16).to(DEV)
    rd = res.to(torch.bfloat16).to(DEV) if with_res else None
    N.check(lib().ctta_lrelu_bwd(N.ptr(gd), N.ptr(ad), slope, alpha, N.ptr(rd), N.ptr(out), n, accumulate, N.stream_ptr()))
    sync()
    assert bool((out[n:].float() == POISON).all())
    assert_bf16_close(out[:n].float().cpu(), ref, (tag, n, slope, with_res, accumulate))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("slope", [0.1, 0.01])
def test_lrelu_bwd(slope, with_res, accumulate):
    """out (+)= res + alpha g (act > 0 ? 1 : slope); act = +0 and -0 take the slope."""
    for n in (8, 8 * 257):
        _lrelu_case(n, slope, with_res, accumulate, "lr")


def test_lrelu_bwd_second_grid_stride_trip():
    cap = launcher_block_cap("lrelu_bwd_kernel")
    _lrelu_case((cap * 256 + 300) * 8, 0.1, True, 1, "lrb")


def test_lrelu_bwd_refuses_a_ragged_length():
    t = torch.zeros(16, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        N.check(lib().ctta_lrelu_bwd(N.ptr(t), N.ptr(t), 0.1, 1.0, None, N.ptr(t), 12, 0, N.stream_ptr()))


# ------------------------------------------------------------------------------------ table-driven transposes / copies
def _run_transposes(specs):
    """specs: (rows, cols, src_ld, wcols, dst_ld); the table is built as WeightPacker::add_transpose builds it."""
    jobs = (N.TposeJob * len(specs))()
    keep, blocks = [], 0
    for i, (rows, cols, src_ld, wcols, dst_ld) in enumerate(specs):
        src = torch.full((rows, src_ld), POISON)
        src[:, :cols] = bf16_round(det("tp.%d" % i, (rows, cols), i + 1))
        srcd = src.to(torch.bfloat16).to(DEV)
        dstd = torch.full((cols + 1, dst_ld), POISON, dtype=torch.bfloat16, device=DEV)   # one guard row
        want = torch.full((cols + 1, dst_ld), POISON)
        want[:cols, :wcols] = 0.0
        want[:cols, :rows] = src[:, :cols].T
        j = jobs[i]
        j.src, j.dst, j.rows, j.cols, j.src_ld, j.dst_ld, j.wcols = srcd.data_ptr(), dstd.data_ptr(), rows, cols, src_ld, dst_ld, wcols
        j.block0, j.tiles_r = blocks, (wcols + 63) // 64
        blocks += j.tiles_r * ((cols + 63) // 64)
        keep.append((srcd, dstd, want.to(torch.bfloat16)))
    table = upload_table(jobs)
    N.check(lib().ctta_transpose_multi(N.ptr(table), len(specs), blocks, N.stream_ptr()))
    sync()
    for i, (_, dstd, want) in enumerate(keep):
        assert torch.equal(dstd.cpu().view(torch.int16), want.view(torch.int16)), specs[i]


def test_transpose_multi():
    """dst[c][r] = src[r][c]; columns rows .. wcols-1 zero; columns behind wcols (dst_ld > wcols) not written."""
    specs = [(64, 64, 64, 64, 72),        # whole tile, dst_ld > wcols
             (1, 8, 8, 8, 8),             # one row: wcols > rows
             (70, 136, 144, 72, 72),      # ragged both ways, wcols > rows, source rows longer than cols
             (200, 72, 72, 200, 208)]     # several row tiles, dst_ld > wcols
    assert ctypes.sizeof(N.TposeJob) == 48
    _run_transposes(specs)
    _run_transposes(specs[2:3])           # a single-job table (the binary search over one entry)
    _run_transposes(list(reversed(specs)))


def test_copy_segments_multi():
    counts = [1, 255, 0, 256, 257, 1000]
    gap = 5
    src = det("cs.src", (sum(counts) + 3,), 1)
    total = sum(c + gap for c in counts) + gap
    want = torch.full((total,), POISON)
    srcd, dstd = src.to(DEV), want.clone().to(DEV)
    segs = (N.CopySeg * len(counts))()
    s_off, d_off = 3, gap                 # sources start 12 bytes into the buffer: no 16-byte alignment is promised
    for i, c in enumerate(counts):
        segs[i].src, segs[i].dst, segs[i].count = srcd.data_ptr() + 4 * s_off, dstd.data_ptr() + 4 * d_off, c
        want[d_off:d_off + c] = src[s_off:s_off + c]
        s_off += c
        d_off += c + gap
    assert ctypes.sizeof(N.CopySeg) == 24
    table = upload_table(segs)
    N.check(lib().ctta_copy_segments_multi(N.ptr(table), len(counts), N.stream_ptr()))
    sync()
    assert torch.equal(dstd.cpu(), want)  # the gaps between (and around) the destination ranges keep their poison


# ------------------------------------------------------------------------------------ layout moves / conversions
@pytest.mark.parametrize("B,C,HW,cs", [(2, 8, 35, 8), (3, 5, 129, 8)])
def test_nhwc_f32_to_nchw_f32(B, C, HW, cs):
    src = det("nf.x", (B, HW, cs), 1)
    dst = torch.full((B * C * HW + 7,), POISON, device=DEV)
    srcd = src.to(DEV)
    N.check(lib().ctta_nhwc_f32_to_nchw_f32(N.ptr(srcd), N.ptr(dst), B, C, HW, cs, N.stream_ptr()))
    sync()
    want = torch.cat([src[:, :, :C].permute(0, 2, 1).reshape(-1), torch.full((7,), POISON)])
    assert torch.equal(dst.cpu(), want)


@pytest.mark.parametrize("rows,cols,cols_pad", [(7, 64, 64), (5, 61, 64), (3, 1, 8)])
def test_rows_f32_to_bf16_rounds_like_torch(rows, cols, cols_pad):
    special = torch.tensor([1.0 + 2.0 ** -8,          # tie: down to the even 1.0
                            1.0 + 3 * 2.0 ** -8,      # tie: up to the even 1 + 2^-6
                            -0.0,
                            1e-40,                    # fp32 subnormal, a bf16 subnormal too
                            0.0,
                            3.4028234663852886e38,    # FLT_MAX: the largest finite value, rounds to +inf
                            -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8), -3.4028234663852886e38,
                            3.3895313892515355e38,    # bf16's own largest finite value stays
                            2.0 ** -133, 1.4e-45, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 - 2.0 ** -20],
                           dtype=torch.float32)
    x = det("rb.x", (rows * cols,), 1) * 3.0
    k = min(len(special), x.numel())
    x[:k] = special[:k]
    x = x.reshape(rows, cols)
    want = torch.zeros(rows, cols_pad, dtype=torch.bfloat16)
    want[:, :cols] = x.to(torch.bfloat16)
    if k == len(special):
        assert bool(torch.isinf(want.view(-1)[5])) and float(want.view(-1)[3]) != 0.0   # the reference itself sees them
    dst = torch.full((rows * cols_pad + 8,), POISON, dtype=torch.bfloat16, device=DEV)
    xd = x.to(DEV)
    N.check(lib().ctta_rows_f32_to_bf16(N.ptr(xd), N.ptr(dst), rows, cols, cols_pad, N.stream_ptr()))
    sync()
    got = dst.cpu()
    assert bool((got[rows * cols_pad:].float() == POISON).all())
    assert torch.equal(got[:rows * cols_pad].view(torch.int16), want.view(-1).view(torch.int16))


def test_rows_f32_to_bf16_refuses_an_unpadded_row():
    x = torch.zeros(3 * 12, device=DEV)
    dst = torch.zeros(3 * 12, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        N.check(lib().ctta_rows_f32_to_bf16(N.ptr(x), N.ptr(dst), 3, 12, 12, N.stream_ptr()))


# ------------------------------------------------------------------------------------ weighted MSE
@pytest.mark.parametrize("n", [4, 1028, 4 * 256 * 3 + 4])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("weighted", [False, True])
def test_weighted_mse_loss(weighted, B, n):
    """mean_b(w_b mean((p - t)^2)): one vector per instance, one trip + 1 vector, three trips + 1 vector of the 256 lanes."""
    p, t = det("wm.p", (B, n), 1), det("wm.t", (B, n), 2) * 0.7
    w = det("wm.w", (B,), 3).abs() + 0.25 if weighted else None
    inst64 = ((p.double() - t.double()) ** 2).mean(dim=1)
    loss64 = float(((w.double() if weighted else 1.0) * inst64).mean())
    inst = torch.full((B + 1,), POISON, device=DEV)
    loss = torch.full((2,), POISON, device=DEV)
    pd, td, wd = p.to(DEV), t.to(DEV), (w.to(DEV) if weighted else None)
    N.check(lib().ctta_weighted_mse_loss(N.ptr(pd), N.ptr(td), N.ptr(wd), N.ptr(inst), N.ptr(loss), B, n, N.stream_ptr()))
    sync()
    inst, loss = inst.cpu().double(), loss.cpu().double()
    assert float(inst[B]) == POISON and float(loss[1]) == POISON
    assert float(((inst[:B] - inst64).abs() / inst64).max()) <= 1e-5
    assert abs(float(loss[0]) - loss64) <= 1e-5 * abs(loss64)


def test_weighted_mse_loss_refuses_a_ragged_sample():
    t = torch.zeros(16, device=DEV)
    with pytest.raises(RuntimeError):
        N.check(lib().ctta_weighted_mse_loss(N.ptr(t), N.ptr(t), None, N.ptr(t), N.ptr(t), 2, 6, N.stream_ptr()))


@pytest.mark.parametrize("weighted", [False, True])
def test_weighted_mse_grad(weighted):
    """d loss / d pred, scaled by loss_scale, as NHWC bf16 with c_pad > c: the pad lanes are exactly zero."""
    B, C, HW, cpad, loss_scale = 3, 5, 35, 8, 1024.0
    p, t = det("wg.p", (B, C, HW), 1), det("wg.t", (B, C, HW), 2) * 0.7
    w = det("wg.w", (B,), 3).abs() + 0.25 if weighted else None
    pp = p.double().requires_grad_(True)
    inst = ((pp - t.double()) ** 2).reshape(B, -1).mean(dim=1)
    (((w.double() if weighted else 1.0) * inst).mean() * loss_scale).backward()
    ref = pp.grad.permute(0, 2, 1)                            # (B, HW, C)
    out = torch.full((B * HW * cpad + 8,), POISON, dtype=torch.bfloat16, device=DEV)
    pd, td, wd = p.to(DEV), t.to(DEV), (w.to(DEV) if weighted else None)
    N.check(lib().ctta_weighted_mse_grad(N.ptr(pd), N.ptr(td), N.ptr(wd), loss_scale, B, C, HW, cpad, N.ptr(out), N.stream_ptr()))
    sync()
    got = out.float().cpu()
    assert bool((got[B * HW * cpad:] == POISON).all())
    got = got[:B * HW * cpad].reshape(B, HW, cpad)
    assert float(got[..., C:].abs().max()) == 0.0
    assert_bf16_close(got[..., :C], ref, "weighted_mse_grad")


# ------------------------------------------------------------------------------------ gradient scatters
def _offsets(name, n, span, seed, drop):
    """n distinct offsets in [0, span), every `drop`-th one negative (= skipped)."""
    order = np.argsort(det(name, (span,), seed).numpy(), kind="stable")[:n].astype(np.int32)
    order[::drop] = -1
    return torch.from_numpy(order.copy())


# Bound of the scatters: 1e-6 relative to the sum of magnitudes that meet in an entry.  The kernels add the S slabs in
# fp32 in slab order, then (accumulate) once more: each addition rounds to 2^-24 of a partial sum that never exceeds
# that sum of magnitudes, so S + 1 <= 16 additions stay inside 1e-6 of it whatever the data, and the 18 of S = 17 would
# have to round the same way at full size every time to leave it.


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("S", [1, 8, 9, 17])
def test_wgrad_scatter(S, accumulate):
    """grad_w[row_off[n] + col_off[k]] (+)= sum_s slab[s][k][n] through the tiled kernel (col_off given / NULL) and the
    generic kernel with the aux mask; S = 8 / 9 / 17 cover the eight-in-flight body of the slab sum and its tail."""
    K, Nc, ldn, extra = 70, 75, 80, 2
    row_len = 96
    slabs = det("ws.s", (S, K + extra, ldn), S)
    slabs64 = slabs.double()[:, :K, :Nc]                      # [S][k][n]
    row_off = _offsets("ws.ro", Nc, Nc + 4, 1, 9)
    row_off = torch.where(row_off >= 0, row_off * row_len, row_off)
    col_perm = _offsets("ws.co", K, row_len, 2, 11)
    row_aux = torch.from_numpy((np.arange(Nc) % 7).astype(np.int32))
    col_aux = torch.from_numpy((np.arange(K) % 5).astype(np.int32))
    aux_limit = 8
    size = (Nc + 4) * row_len
    start = det("ws.g", (size,), 3) if accumulate else torch.full((size,), POISON)
    sd, rod, rad, cad = slabs.to(DEV), row_off.to(DEV), row_aux.to(DEV), col_aux.to(DEV)
    ro_l, ra_l, ca_l = row_off.tolist(), row_aux.tolist(), col_aux.tolist()
    for mode in ("col_off", "identity", "aux"):
        co = torch.arange(K, dtype=torch.int32) if mode == "identity" else col_perm
        co_l = co.tolist()
        want = start.double().clone()
        tol = torch.zeros(size, dtype=torch.float64)
        written = torch.zeros(size, dtype=torch.bool)
        for n in range(Nc):
            for k in range(K):
                if ro_l[n] < 0 or co_l[k] < 0:
                    continue
                if mode == "aux" and ra_l[n] + ca_l[k] >= aux_limit:
                    continue
                j = ro_l[n] + co_l[k]
                assert not written[j]
                written[j] = True
                v = 0.0
                for s in range(S):
                    v += float(slabs64[s, k, n])
                prev = float(want[j]) if accumulate else 0.0
                want[j] = prev + v
                tol[j] = 1e-6 * (float(slabs64[:, k, n].abs().sum()) + abs(prev))
        assert 0 < int(written.sum()) < K * Nc
        grad = start.clone().to(DEV)
        cod = col_perm.to(DEV) if mode != "identity" else None
        aux = mode == "aux"
        N.check(lib().ctta_wgrad_scatter(N.ptr(sd), S, (K + extra) * ldn, ldn, K, Nc, N.ptr(rod), N.ptr(cod),
                                         N.ptr(rad) if aux else None, N.ptr(cad) if aux else None,
                                         aux_limit if aux else 0, N.ptr(grad), accumulate, N.stream_ptr()))
        sync()
        got = grad.cpu()
        assert torch.equal(got[~written], start[~written]), mode      # skipped entries keep what they held
        excess = (got.double() - want).abs() - tol
        assert float(excess[written].max()) <= 0.0, (mode, float(excess[written].max()))


def test_wgrad_scatter_aux_needs_a_column_map():
    t = torch.zeros(64, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        N.check(lib().ctta_wgrad_scatter(N.ptr(t), 1, 64, 8, 8, 8, N.ptr(i), None, N.ptr(i), N.ptr(i), 4, N.ptr(t), 0,
                                         N.stream_ptr()))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("S", [1, 8, 9, 17])
def test_row_scatter(S, accumulate):
    """dst[idx[n]] (+)= sum_s slab[s][row][n] (the bias row behind a weight slab), idx given / NULL; 300 columns = two blocks."""
    K, Nc, ldn = 6, 300, 304
    row = K                                                   # the extra row behind the k_rows weight rows
    slabs = det("rs.s", (S, K + 2, ldn), S)
    col64 = slabs.double()[:, row, :Nc]                       # [S][n]
    size = Nc + 9
    start = det("rs.d", (size,), 3) if accumulate else torch.full((size,), POISON)
    sd = slabs.to(DEV)
    for idx in (_offsets("rs.i", Nc, size, 4, 13), None):
        want = start.double().clone()
        tol = torch.zeros(size, dtype=torch.float64)
        written = torch.zeros(size, dtype=torch.bool)
        for n in range(Nc):
            j = int(idx[n]) if idx is not None else n
            if j < 0:
                continue
            v = 0.0
            for s in range(S):
                v += float(col64[s, n])
            prev = float(want[j]) if accumulate else 0.0
            want[j] = prev + v
            tol[j] = 1e-6 * (float(col64[:, n].abs().sum()) + abs(prev))
            written[j] = True
        dst = start.clone().to(DEV)
        idxd = idx.to(DEV) if idx is not None else None
        N.check(lib().ctta_row_scatter(N.ptr(sd), S, (K + 2) * ldn, ldn, row, Nc, N.ptr(idxd), N.ptr(dst), accumulate,
                                       N.stream_ptr()))
        sync()
        got = dst.cpu()
        assert 0 < int(written.sum()) < size
        assert torch.equal(got[~written], start[~written])
        excess = (got.double() - want).abs() - tol
        assert float(excess[written].max()) <= 0.0, float(excess[written].max())
