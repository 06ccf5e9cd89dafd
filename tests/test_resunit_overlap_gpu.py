"""The overlapped schedule of the fused HiFi-GAN ResBlock unit (csrc/resunit.hip, CTTA_RESUNIT_OVERLAP): every staging load of
a tile in flight at once (rows past the tile pushed out of the descriptor's range), weight fragments, biases and the
epilogue's first residual rows requested one phase early, position fragments read two blocks ahead of their MFMAs (the
last reads of a K loop must not run past it).  What such a schedule can break is WHICH rows a tile stages and
which tile, sample or launch a prefetched value belongs to, so the cases sit where that changes: tile counts around the CU
count (one workgroup per CU at C = 256 / 512, so grid - 1 / grid / grid + 1 / 2 grid + 1 tiles are one round less one, one
round, and the first tiles of a second and third round), tiles whose successor lies in the next sample, the largest accepted
dilations (no LDS row to spare), the stage-fold epilogue over many tiles, and capture into a graph.

Reference: F.conv1d (CPU fp32) on bf16-rounded operands with the intermediate rounded to bf16; bound: rel_err < 2 * BF16_TOL,
the bound of test_ops_gpu.py::test_fused_resblock_unit.  Where two launches must agree they must agree bit for bit."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from consistencytta_amd import _native as N
from gpu_util import DEV, bf16_round, det, pack_conv_weight, rel_err, sync
from resunit_range import D_MAX, resunit_geom

pytestmark = pytest.mark.gpu

BF16_TOL = 1.5 * 2.0 ** -8      # tests/test_ops_gpu.py


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def weights(C, k):
    """(w1, b1, w2, b2) on the host (bf16-rounded fp32) and (w1 fragments, b1, w2 fragments, b2) on the device"""
    w1 = bf16_round(det("ro.w1", (C, C, k), 2) * (1.0 / math.sqrt(C * k)))
    w2 = bf16_round(det("ro.w2", (C, C, k), 3) * (1.0 / math.sqrt(C * k)))
    b1, b2 = det("ro.b1", (C,), 4) * 0.1, det("ro.b2", (C,), 5) * 0.1
    frags = []
    for w in (w1, w2):
        wp, k_pad = pack_conv_weight(w[:, :, None, :])
        f = torch.empty(C * k * C, dtype=torch.bfloat16, device=DEV)
        N.check(N.lib().ctta_frag_pack(N.ptr(wp), C, k_pad, k * C, N.ptr(f), N.stream_ptr()))
        frags.append(f)
    sync()
    return (w1, b1, w2, b2), (frags[0], b1.to(DEV), frags[1], b2.to(DEV))


def unit_ref(x, C, k, d):
    """x: (B, C, L) bf16-rounded fp32 -> x + conv2(lrelu(conv1(lrelu(x)))), the intermediate rounded to bf16"""
    w1, b1, w2, b2 = weights(C, k)[0]
    mid = bf16_round(F.leaky_relu(F.conv1d(F.leaky_relu(x, 0.1), w1, b1, dilation=d, padding=(k * d - d) // 2), 0.1))
    return x + F.conv1d(mid, w2, b2, padding=(k - 1) // 2)


def to_dev(x):
    return x.permute(0, 2, 1).contiguous().to(torch.bfloat16).to(DEV)


def from_dev(y):
    return y.float().permute(0, 2, 1).cpu()


def launch(xa, C, k, d, out=None, accumulate=0, alpha=1.0, out_slope=0.0):
    """xa: (B, L, C) bf16 on the device"""
    B, L = xa.shape[0], xa.shape[1]
    f1, b1, f2, b2 = weights(C, k)[1]
    if out is None:
        out = torch.full_like(xa, float("nan"))
    N.check(N.lib().ctta_resunit_conv1d(N.ptr(xa), B, L, C, k, d, N.ptr(f1), N.ptr(b1), N.ptr(f2), N.ptr(b2), 0.1, N.ptr(out),
                                        accumulate, alpha, out_slope, N.stream_ptr()))
    return out


def check_unit(C, k, d, B, L, tag):
    assert N.lib().ctta_resunit_supported(C, k, d) == 1
    x = bf16_round(det("ro.x." + tag, (B, C, L), 1))
    out = launch(to_dev(x), C, k, d)
    sync()
    err = rel_err(from_dev(out), unit_ref(x, C, k, d))
    print("C %d k %d d %d B %d L %d: rel_err %.3e (bound %.3e)" % (C, k, d, B, L, err, 2 * BF16_TOL))
    assert err < 2 * BF16_TOL


WALK = ("one", "grid-1", "grid", "grid+1", "2grid+1")


@pytest.mark.parametrize("tiles", WALK)
@pytest.mark.parametrize("C,k,d", [(256, 7, 3), (512, 3, 1)])
def test_tile_counts_around_the_cu_count(C, k, d, tiles):
    """B = 1, L = T * (tiles - 1) + 1: the last tile is one position long and has no successor; with more tiles than CUs a CU
    takes a second (third) tile after its first."""
    g = cu_count()
    n = {"one": 1, "grid-1": g - 1, "grid": g, "grid+1": g + 1, "2grid+1": 2 * g + 1}[tiles]
    T = resunit_geom(C, k, d)[0]
    check_unit(C, k, d, 1, T * (n - 1) + 1, "walk")


@pytest.mark.parametrize("k,d", [(3, 1), (7, 3), (11, 5)])
@pytest.mark.parametrize("C", [32, 64, 128, 256, 512])
def test_next_tile_lies_in_the_next_sample(C, k, d):
    """Two tiles per sample with a one-position second tile (B = 3), one partial tile per sample (B = 5) and one-position
    samples: whatever follows a sample's last tile belongs to another sample."""
    T = resunit_geom(C, k, d)[0]
    check_unit(C, k, d, 3, T + 1, "sb")
    check_unit(C, k, d, 5, T - 5, "sb")
    check_unit(C, k, d, 3, 1, "sb")


@pytest.mark.parametrize("C,k,d,T", [(256, 11, 7, 224), (256, 3, 51, 192), (512, 11, 6, 80), (512, 7, 10, 80), (512, 3, 38, 64)])
def test_largest_dilations_of_the_eight_wave_forms(C, k, d, T):
    """The tile fills the LDS: no row is free for anything but the tile itself.  2.5 tiles per sample, B = 2."""
    assert D_MAX[(C, k)] == d and resunit_geom(C, k, d)[0] == T
    check_unit(C, k, d, 2, 2 * T + T // 2, "dmax")


@pytest.mark.parametrize("C,k,d,per_cu", [(256, 3, 1, 1), (64, 3, 1, 3)])
def test_stage_fold_over_three_rounds_of_tiles(C, k, d, per_cu):
    """accumulate = 1, alpha = 1/3, out_slope = 0.01 with more than three tiles per resident workgroup: the old output and
    the residual requested ahead of conv2 belong to the tile that is finished."""
    T = resunit_geom(C, k, d)[0]
    B, n = 3, cu_count() * per_cu + 1                     # tiles per sample: 3 n > 3 * resident workgroups
    L = T * (n - 1) + 1
    x = bf16_round(det("ro.x.fold", (B, C, L), 1))
    old = bf16_round(det("ro.o.fold", (B, C, L), 6))
    out = launch(to_dev(x), C, k, d, out=to_dev(old), accumulate=1, alpha=1.0 / 3.0, out_slope=0.01)
    sync()
    ref = F.leaky_relu((old + unit_ref(x, C, k, d)) / 3.0, 0.01)
    err = rel_err(from_dev(out), ref)
    print("C %d fold, %d tiles: rel_err %.3e (bound %.3e)" % (C, B * n, err, 2 * BF16_TOL))
    assert err < 2 * BF16_TOL


@pytest.mark.parametrize("C,k,d", [(256, 7, 3), (512, 3, 1), (64, 7, 3)])
def test_a_sample_does_not_depend_on_its_place_in_the_launch(C, k, d):
    """A sample alone (B = 1) and as the second of three (other workgroups, other positions in a CU's sequence of tiles)
    gives the same bits; so do two launches in a row."""
    T = resunit_geom(C, k, d)[0]
    L = T * (cu_count() // 2) + 7
    x3 = to_dev(bf16_round(det("ro.x.ind", (3, C, L), 1)))
    out3 = launch(x3, C, k, d)
    again = launch(x3, C, k, d)
    out1 = launch(x3[1:2].contiguous(), C, k, d)
    sync()
    assert not torch.isnan(out3.float()).any()
    assert torch.equal(out3, again)
    assert torch.equal(out1[0], out3[1])


def test_two_units_captured_in_one_graph():
    """unit(unit(x)) captured on one stream and replayed three times against the eager result."""
    C, k, d = 256, 7, 3
    T = resunit_geom(C, k, d)[0]
    x = to_dev(bf16_round(det("ro.x.graph", (2, C, 3 * T + 5), 1)))
    y, z = torch.empty_like(x), torch.empty_like(x)
    launch(x, C, k, d, out=y)
    launch(y, C, k, 1, out=z)
    sync()
    eager = z.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                               # warm-up on the side stream, as torch asks before a capture
        launch(x, C, k, d, out=y)
        launch(y, C, k, 1, out=z)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(x, C, k, d, out=y)
        launch(y, C, k, 1, out=z)
    for _ in range(3):
        y.fill_(float("nan"))
        z.fill_(float("nan"))
        graph.replay()
        sync()
        assert torch.equal(z, eager)
