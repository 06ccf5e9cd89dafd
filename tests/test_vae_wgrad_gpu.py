"""Parameter-gradient operators of the VAE decoder's backward vs torch autograd on the CPU (the same bf16-rounded inputs,
fp32 reference, the 2e-3 bound of test_bwd_ops_gpu.py): the implicit 3x3 weight gradient at image width 64 in its three
operand forms, conv_out's one-output-channel weight / bias gradient and post_quant_conv's."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from consistencytta_amd import _native as N  # noqa: E402
from gpu_util import DEV, bf16_round, det, nhwc_bf16, rel_err, sync  # noqa: E402

TOL = 2e-3          # fp32 accumulation of bf16 products (tests/test_bwd_ops_gpu.py)


def lib():
    return N.lib()


def rup(a, b):
    return (a + b - 1) // b * b


@pytest.mark.parametrize("B,H,W,Cin,Cout,splits,nb", [(1, 1, 64, 32, 8, 1, 0), (2, 2, 64, 40, 72, 1, 2),
                                                      (1, 3, 64, 64, 64, 2, 0), (2, 4, 64, 128, 128, 4, 0)])
def test_implicit_weight_gradient_at_width_64(B, H, W, Cin, Cout, splits, nb):
    """wgrad_implicit_w64_kernel through ctta_wgrad_implicit / _inplace / _direct: one image row per 64-position chunk, a
    3 x 66 bordered patch.  One row alone (both vertical borders zero, smallest c and n); a sample boundary between chunks
    with ragged channel blocks, a ragged output tile and per-sample columns; M = 192 padded to mp = 256 (zero positions
    inside a split); the decoder level's own widths."""
    L = lib()
    st = N.stream_ptr()
    x = bf16_round(det("w64.x", (B, Cin, H, W), 1)).requires_grad_(True)
    w = bf16_round(det("w64.w", (Cout, Cin, 3, 3), 2) / math.sqrt(Cin * 9)).requires_grad_(True)
    b = (det("w64.b", (Cout,), 3) * 0.1).requires_grad_(True)
    y = F.conv2d(x, w, b, padding=1)
    dy = bf16_round(det("w64.dy", tuple(y.shape), 4))
    y.backward(dy)
    xa, dya = nhwc_bf16(x.detach()), nhwc_bf16(dy)
    M, K = B * H * W, 9 * Cin
    assert L.ctta_wgrad_implicit_supported(9, Cin, H, W, Cin, Cout) == 1
    # what was outside the range stays outside
    assert L.ctta_wgrad_implicit_supported(9, 64, 8, 48, 64, 64) == 0 and L.ctta_wgrad_implicit_supported(9, 64, 6, 4, 64, 64) == 0
    assert L.ctta_wgrad_implicit_supported(9, 64, 8, 128, 64, 64) == 0 and L.ctta_wgrad_implicit_supported(9, 24, 8, 64, 24, 64) == 0
    mp = rup(M, 64 * splits)
    pt = torch.empty(Cout, mp, dtype=torch.bfloat16, device=DEV)
    N.check(L.ctta_transpose_bf16(N.ptr(dya), 0, M, Cout, Cout, 0, N.ptr(pt), 0, mp, 1, st))
    ld = rup(K + 1 + nb, 4)
    # slab form, dY^T operand
    slabs = torch.full((splits, Cout, ld), float("nan"), device=DEV)
    N.check(L.ctta_wgrad_implicit(N.ptr(pt), Cout, mp, N.ptr(xa), Cin, Cin, B, H, W, 9, M, splits, K, nb, N.ptr(slabs),
                                  Cout * ld, ld, st))
    sync()
    got = slabs[:, :, :K + 1 + nb].sum(0).cpu()
    assert torch.isfinite(slabs[:, :, :K + 1 + nb]).all()
    assert rel_err(got[:, :K].reshape(Cout, Cin, 3, 3), w.grad) < TOL
    assert rel_err(got[:, K], b.grad) < TOL
    if nb:
        assert rel_err(got[:, K + 1:K + 1 + nb].t(), dy.sum(dim=(2, 3))[:nb]) < TOL
    # dY read where it lies: the same MFMA products in the same order, slab by slab
    slabs2 = torch.full((splits, Cout, ld), float("nan"), device=DEV)
    N.check(L.ctta_wgrad_implicit_inplace(N.ptr(dya), Cout, Cout, mp, N.ptr(xa), Cin, Cin, B, H, W, 9, M, splits, K, nb,
                                          N.ptr(slabs2), Cout * ld, ld, st))
    sync()
    assert torch.equal(slabs2[:, :, :K], slabs[:, :, :K])
    got2 = slabs2[:, :, :K + 1 + nb].sum(0).cpu()
    assert torch.isfinite(got2).all()
    assert rel_err(got2[:, K], b.grad) < TOL
    if nb:
        assert rel_err(got2[:, K + 1:K + 1 + nb].t(), dy.sum(dim=(2, 3))[:nb]) < TOL
    # one split added straight into the gradient tensors = slab + scatter (accumulate), padded rows and bias slots dropped
    mp1 = rup(M, 64)
    ld1 = rup(K + 1, 4)
    slab1 = torch.full((1, Cout, ld1), float("nan"), device=DEV)
    N.check(L.ctta_wgrad_implicit_inplace(N.ptr(dya), Cout, Cout, mp1, N.ptr(xa), Cin, Cin, B, H, W, 9, M, 1, K, 0,
                                          N.ptr(slab1), Cout * ld1, ld1, st))
    ro = torch.arange(Cout, dtype=torch.int32) * K
    bidx = torch.arange(Cout, dtype=torch.int32)
    ro[1], bidx[2] = -1, -1
    ro_d, bi_d = ro.to(DEV), bidx.to(DEV)
    gw0, gb0 = det("w64.gw", (Cout * K,), 8).to(DEV), det("w64.gb", (Cout,), 9).to(DEV)
    gw_s, gb_s, gw_d, gb_d = gw0.clone(), gb0.clone(), gw0.clone(), gb0.clone()
    N.check(L.ctta_wgrad_scatter_rows_bias(N.ptr(slab1), 1, Cout * ld1, ld1, K, Cout, N.ptr(ro_d), None, N.ptr(gw_s), K, Cout,
                                           N.ptr(bi_d), N.ptr(gb_s), 1, st))
    N.check(L.ctta_wgrad_implicit_direct(N.ptr(dya), Cout, Cout, mp1, N.ptr(xa), Cin, Cin, B, H, W, M, K, Cout, N.ptr(ro_d),
                                         N.ptr(gw_d), Cout, N.ptr(bi_d), N.ptr(gb_d), st))
    sync()
    assert torch.equal(gw_d, gw_s) and torch.equal(gb_d, gb_s)
    assert torch.equal(gw_d.view(Cout, K)[1], gw0.view(Cout, K)[1]) and float(gb_d[2]) == float(gb0[2])
    assert rel_err((gw_d - gw0).cpu().view(Cout, K)[2:].reshape(Cout - 2, Cin, 3, 3), w.grad[2:]) < TOL


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 8), (2, 3, 5, 40), (3, 16, 32, 256)])
def test_upsample2_nearest(B, H, W, C):
    """ctta_upsample2_nearest: the materialised x2 input of the upsampling convolutions' weight gradient, bit for bit."""
    x = det("up2.x", (B, H, W, C), 1).to(torch.bfloat16).to(DEV)
    out = torch.full((B, 2 * H, 2 * W, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    N.check(lib().ctta_upsample2_nearest(N.ptr(x), N.ptr(out), B, H, W, C, N.stream_ptr()))
    sync()
    assert torch.equal(out, x.repeat_interleave(2, 1).repeat_interleave(2, 2))


@pytest.mark.parametrize("B,H,W,C", [(2, 4, 8, 32), (1, 3, 5, 32), (2, 8, 64, 128)])
def test_conv_out_weight_and_bias_gradient(B, H, W, C):
    """ctta_conv_cout1_wgrad (csrc/backward.hip): dW / db of F.conv2d(a, w (1, C, 3, 3), b, padding=1) for an fp32 upstream
    gradient; one workgroup, sizes at which every border tap clips, several workgroups (1024 pixels at C = 128).  Fixed
    summation order: two runs give the same bits; accumulate = 1 adds to what the buffers hold."""
    L = lib()
    st = N.stream_ptr()
    a = bf16_round(det("co.a", (B, C, H, W), 1))
    w = (det("co.w", (1, C, 3, 3), 2) / math.sqrt(C * 9)).requires_grad_(True)
    b = torch.zeros(1, requires_grad=True)
    gy = det("co.gy", (B, 1, H, W), 3)
    F.conv2d(a, w, b, padding=1).backward(gy)
    n = L.ctta_conv_cout1_wgrad_scratch_floats(B, H, W, 3, 3, C)
    assert n >= 9 * C + 1
    scratch = torch.full((n,), float("nan"), device=DEV)
    ad, gyd = nhwc_bf16(a), gy.to(DEV).contiguous()
    runs = []
    for _ in range(2):
        dw, db = torch.full((1, C, 3, 3), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
        N.check(L.ctta_conv_cout1_wgrad(N.ptr(gyd), N.ptr(ad), B, H, W, 3, 3, 1, 1, C, N.ptr(dw), N.ptr(db), 0, N.ptr(scratch), st))
        sync()
        runs.append((dw, db))
    (dw, db), (dw2, db2) = runs
    assert rel_err(dw, w.grad) < TOL and rel_err(db, b.grad) < TOL
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    N.check(L.ctta_conv_cout1_wgrad(N.ptr(gyd), N.ptr(ad), B, H, W, 3, 3, 1, 1, C, N.ptr(dw2), N.ptr(db2), 1, N.ptr(scratch), st))
    sync()
    assert torch.equal(dw2, dw + dw) and torch.equal(db2, db + db)
    with pytest.raises(RuntimeError):      # more taps than the kernel holds: refused
        N.check(L.ctta_conv_cout1_wgrad(N.ptr(gyd), N.ptr(ad), B, H, W, 1, 10, 0, 4, C, N.ptr(dw), N.ptr(db), 0, N.ptr(scratch), st))


@pytest.mark.parametrize("B,HW,ld", [(2, 16, 8), (3, 100, 16)])
def test_post_quant_conv_gradient(B, HW, ld):
    """ctta_post_quant_wgrad: dW / db of post_quant_conv (1x1, 8 -> 8) applied to z / scale, from the bf16 gradient of its
    output as the decoder's backward leaves it (NHWC, ld elements per pixel) and the fp32 latent; a single partial tile,
    and three tiles with sample boundaries inside them."""
    L = lib()
    st = N.stream_ptr()
    zin = zout = 8
    inv_scale = 1.0 / 0.9
    z = det("pq.z", (B, zin, HW, 1), 1)
    w = (det("pq.w", (zout, zin, 1, 1), 2) / math.sqrt(zin)).requires_grad_(True)
    b = torch.zeros(zout, requires_grad=True)
    dz = bf16_round(det("pq.dz", (B, zout, HW, 1), 3))
    F.conv2d(z * inv_scale, w, b).backward(dz)
    dzd = torch.full((B * HW, ld), float("nan"), dtype=torch.bfloat16, device=DEV)
    dzd[:, :zout] = dz.permute(0, 2, 3, 1).reshape(B * HW, zout).to(torch.bfloat16).to(DEV)
    zd = z.reshape(B, zin, HW).contiguous().to(DEV)
    n = L.ctta_post_quant_wgrad_scratch_floats(B, HW, zin, zout)
    assert n >= zout * zin + zout
    scratch = torch.full((n,), float("nan"), device=DEV)
    runs = []
    for _ in range(2):
        dw, db = torch.full((zout, zin, 1, 1), float("nan"), device=DEV), torch.full((zout,), float("nan"), device=DEV)
        N.check(L.ctta_post_quant_wgrad(N.ptr(dzd), ld, N.ptr(zd), inv_scale, B, zin, zout, HW, N.ptr(dw), N.ptr(db), 0,
                                        N.ptr(scratch), st))
        sync()
        runs.append((dw, db))
    (dw, db), (dw2, db2) = runs
    assert rel_err(dw, w.grad) < TOL and rel_err(db, b.grad) < TOL
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    N.check(L.ctta_post_quant_wgrad(N.ptr(dzd), ld, N.ptr(zd), inv_scale, B, zin, zout, HW, N.ptr(dw2), N.ptr(db2), 1,
                                    N.ptr(scratch), st))
    sync()
    assert torch.equal(dw2, dw + dw) and torch.equal(db2, db + db)
