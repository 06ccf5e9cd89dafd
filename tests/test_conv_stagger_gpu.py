"""The eight-wave 128x64-per-wave tiles of conv_gemm (256x256x64, its stream-K form, 512x128x64) run their two wave halves
out of phase inside a K step (conv_gemm_kernel.h, CTTA_XBAR_STAGGER): waves 4-7 issue the next tile's LDS-DMA behind the
MFMAs they held over the barrier, waves 0-3 in front of them.  Checked here, with `tile` forced to each of the three:
the loop's prologue and drain (1, 2, 3, 4 and 9 K steps), row tiles whose late half is dead or partly dead, two column
tiles, an fp32 output, and that twenty launches in a row give the same bits.  Reference: F.conv2d on bf16-rounded
inputs, tolerance of tests/test_ops_gpu.py (BF16_TOL = 1.5 * 2^-8 of the output's max magnitude; twice that behind the
fused SiLU epilogue, whose input is itself the sum of three rounded terms)."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from consistencytta_amd import _native as N
from gpu_util import DEV, bf16_round, conv_desc, det, from_nhwc, nhwc_bf16, pack_conv_weight, rel_err, sync

pytestmark = pytest.mark.gpu

BF16_TOL = 1.5 * 2.0 ** -8

# variant id -> (rows, columns) of its tile; waves 4-7 own rows BM/2.. of it (wave / WN picks a wave's rows)
STAGGERED = {29: (256, 256), 36: (512, 128), 41: (256, 256)}
_NAMES = {t: N.lib().ctta_conv_gemm_variant_name(t).decode() for t in STAGGERED}
TILES = [pytest.param(t, id=_NAMES[t]) for t in STAGGERED]


def test_the_forced_ids_are_the_eight_wave_tiles():
    assert _NAMES == {29: "256x256x64_w2x4_m2_s2", 36: "512x128x64_w4x2_m2_s2", 41: "256x256x64_w2x4_m2_s2_sk"}


def _case(tile, M, Cin, Cout, k, tag, f32=False, silu=False, reps=1):
    """One sample of M x 1 pixels (M GEMM rows) through the forced tile; returns (error vs F.conv2d, outputs)."""
    pad = (k - 1) // 2
    x = bf16_round(det(tag + ".x", (1, Cin, M, 1), 1))
    w = bf16_round(det(tag + ".w", (Cout, Cin, k, k), 2) * (1.0 / math.sqrt(Cin * k * k)))
    bias = det(tag + ".b", (Cout,), 3) * 0.1
    ref = F.conv2d(x, w, bias, padding=pad)
    wp, k_pad = pack_conv_weight(w)
    xa, bd = nhwc_bf16(x), bias.to(DEV).contiguous()
    kw = dict(x0=xa, c0=Cin, batch=1, hi=M, wi=1, ho=M, wo=1, kh=k, kw=k, pad_h=pad, pad_w=pad, w=wp, k_pad=k_pad, n=Cout,
              bias=bd, ldc=Cout, tile=tile)
    keep = [xa, wp, bd]
    if f32:
        kw.update(out_f32=1)
    if silu:
        rowvec = det(tag + ".rv", (1, Cout), 4) * 0.2
        res = bf16_round(det(tag + ".res", (1, Cout, M, 1), 5))
        ref = F.silu(ref + rowvec[:, :, None, None] + res)
        rv, rs = rowvec.to(DEV).contiguous(), nhwc_bf16(res)
        kw.update(rowvec=rv, rowvec_ld=Cout, res=rs, res_ld=Cout, out_act=1)
        keep += [rv, rs]
    outs = []
    for _ in range(reps):
        out = torch.full((1, M, 1, Cout), float("nan"), dtype=torch.float32 if f32 else torch.bfloat16, device=DEV)
        d = conv_desc(out=out, **kw)
        N.check(N.lib().ctta_conv_gemm(ctypes.byref(d), N.stream_ptr()))       # back to back, no sync in between
        outs.append(out)
    sync()
    return rel_err(from_nhwc(outs[0]), ref), outs


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("cin,k", [(64, 1), (128, 1), (192, 1), (256, 1), (64, 3)], ids=["nk1", "nk2", "nk3", "nk4", "nk9"])
def test_k_loops_of_1_2_3_4_and_9_steps(tile, cin, k):
    """Prologue and drain of the staggered loop: the late half issues no LDS-DMA at all when nk = 1, one behind its first
    (empty) held slot when nk = 2, ...; M = three whole row tiles, every wave live."""
    bm, bn = STAGGERED[tile]
    err, _ = _case(tile, 3 * bm, cin, bn, k, "stg.k%d_%d" % (cin, k))
    print("tile %d cin %d k %d: rel err %.3e (bound %.3e)" % (tile, cin, k, err, BF16_TOL))
    assert err < BF16_TOL


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("cin,k", [(128, 1), (64, 3)], ids=["nk2", "nk9"])
def test_last_row_tile_with_a_dead_late_half(tile, cin, k):
    """M one row past a multiple of the tile's rows: in the last row tile only the first wave row is live, waves 4-7 only
    feed the ring (their LDS-DMA now comes half a step later than the live waves')."""
    bm, bn = STAGGERED[tile]
    err, _ = _case(tile, 2 * bm + 1, cin, bn, k, "stg.dead%d_%d" % (cin, k))
    print("tile %d M %d: rel err %.3e (bound %.3e)" % (tile, 2 * bm + 1, err, BF16_TOL))
    assert err < BF16_TOL


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("cin,k", [(128, 1), (64, 3)], ids=["nk2", "nk9"])
def test_m_ends_inside_the_late_half(tile, cin, k):
    """The last row tile ends at its row bm/2 + bm/8 + 3: the 512-row tile's waves 4-5 (rows 256-383) are live with rows past
    M, its waves 6-7 (rows 384-511) dead; the 256-row tiles' waves 4-7 (rows 128-255) are live with 93 rows past M."""
    bm, bn = STAGGERED[tile]
    M = bm + bm // 2 + bm // 8 + 3
    err, _ = _case(tile, M, cin, bn, k, "stg.part%d_%d" % (cin, k))
    print("tile %d M %d: rel err %.3e (bound %.3e)" % (tile, M, err, BF16_TOL))
    assert err < BF16_TOL


@pytest.mark.parametrize("tile", TILES)
def test_two_column_tiles(tile):
    """N = one whole column tile + 64 channels of a second one, M ragged, nine K steps."""
    bm, bn = STAGGERED[tile]
    err, _ = _case(tile, 2 * bm + 77, 64, bn + 64, 3, "stg.cols")
    print("tile %d N %d: rel err %.3e (bound %.3e)" % (tile, bn + 64, err, BF16_TOL))
    assert err < BF16_TOL


@pytest.mark.parametrize("tile", TILES)
def test_fp32_output(tile):
    bm, bn = STAGGERED[tile]
    err, outs = _case(tile, 2 * bm + 130, 192, bn, 1, "stg.f32", f32=True)
    print("tile %d fp32: rel err %.3e (bound %.3e)" % (tile, err, BF16_TOL))
    assert outs[0].dtype == torch.float32 and err < BF16_TOL


@pytest.mark.parametrize("tile", TILES)
def test_twenty_launches_give_the_same_bits(tile):
    """Back to back on one stream, fused bias + row vector + residual + SiLU epilogue, ragged M, two column tiles."""
    bm, bn = STAGGERED[tile]
    err, outs = _case(tile, 3 * bm + 1, 128, bn + 64, 3, "stg.rep", silu=True, reps=20)
    print("tile %d x20: rel err %.3e (bound %.3e)" % (tile, err, 2 * BF16_TOL))
    assert err < 2 * BF16_TOL
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
