"""CPU-only: the acceptance predicates of the fused HiFi-GAN ResBlock kernels (csrc/resunit.hip) against the region written
out by hand in resunit_range.py.  The engine takes the fused path wherever ctta_resunit_supported says 1, so the table here is
the list of shapes tests/test_resunit_range_gpu.py runs.  Only the predicates are called: nothing here launches a kernel."""
import ctypes
import os
import random

import pytest

from consistencytta_amd import _native as N
from resunit_range import (ANY, D_MAX, LDS_BIG, TILE_SWITCH_512, ChainPredicate, frontier, frontier_picks, raised,
                           reschain_accepted, resunit_fits, resunit_geom, resunit_lds)

WIDTHS = (16, 32, 64, 96, 128, 256, 512, 1024)
HUGE_D = (1000, 10 ** 6, 2 ** 30, 2 ** 31 - 1)     # dil * (k - 1) overflows a 32-bit int from 2^30 on


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    lib = N.lib()
    assert N.get_option("fused_res") == 1       # the predicates answer 0 for everything with the fused path switched off
    return lib


def test_resunit_predicate_matches_the_table(built_lib):
    """ctta_resunit_supported(C, k, d) == (d <= D_MAX[C, k]) for C in WIDTHS, k in 0..13, d in -1..160 and a few huge d."""
    bad = []
    for C in WIDTHS:
        for k in range(14):
            d_max = D_MAX.get((C, k), 0)
            for d in list(range(-1, 161)) + list(HUGE_D):
                want = int(d >= 1 and d <= d_max)
                if built_lib.ctta_resunit_supported(C, k, d) != want:
                    bad.append((C, k, d, want))
    assert not bad, bad[:20]


def test_table_rows_are_the_lds_arithmetic():
    """Every d_max of the table is the last dilation whose tile fits the LDS budget (64 KB at C <= 128, 160 KB at 256 / 512),
    with the tile the launcher picks; at C = 512 the 96-position tile gives way to 64 (k = 3) or 80 (k = 7 / 11) positions."""
    for (C, k), d_max in D_MAX.items():
        if d_max is ANY:
            assert k == 1 and all(resunit_fits(C, k, d) for d in (1, 160) + HUGE_D)
            continue
        assert resunit_fits(C, k, d_max) and not resunit_fits(C, k, d_max + 1), (C, k, d_max)
        assert all(resunit_fits(C, k, d) for d in range(1, d_max + 1)), (C, k)
    for k, d_sw in TILE_SWITCH_512.items():
        assert resunit_lds(512, 1, 96, k, d_sw - 1) <= LDS_BIG < resunit_lds(512, 1, 96, k, d_sw)
        assert resunit_geom(512, k, d_sw - 1)[0] == 96 and resunit_geom(512, k, d_sw)[0] == (64 if k == 3 else 80)
    # k = 7 at d = 8..10 is accepted through the 80-position tile only: the 96-position instance, which the launcher once took
    # for every k = 7, needs (112 + 6 d) * 1 040 B there
    for d in (8, 9, 10):
        assert resunit_lds(512, 1, 80, 7, d) <= LDS_BIG < resunit_lds(512, 1, 96, 7, d) == (112 + 6 * d) * 1040


@pytest.mark.parametrize("C,k", [(32, 3), (32, 5), (32, 7), (64, 3), (64, 5), (64, 7)])
def test_reschain_accepted_set_is_downward_closed_and_walked_exhaustively(built_lib, C, k):
    """Every dilation triple ctta_reschain_supported accepts, by raising d2 until refused, then d1, then d0.  The set is
    downward-closed (lowering any dilation of an accepted triple stays accepted), every triple one step outside it is refused
    (so, downward-closed, no accepted triple lies beyond the walk), random triples of the surrounding box agree with it, and
    HiFi-GAN's (1, 3, 5) is in it.  The frontier -- accepted triples that no single raise keeps accepted -- feeds the GPU test."""
    pred = ChainPredicate(built_lib, C, k)
    acc = reschain_accepted(pred)
    assert (1, 3, 5) in acc and (1, 1, 1) in acc
    for t in acc:
        for i in range(3):
            if t[i] > 1:
                lower = t[:i] + (t[i] - 1,) + t[i + 1:]
                assert lower in acc, (t, lower)
    outside = {r for t in acc for r in raised(t) if r not in acc}
    assert not [r for r in outside if pred(*r)]
    top = max(max(t) for t in acc) + 8
    rng = random.Random(C * 100 + k)
    for _ in range(4000):
        t = tuple(rng.randint(1, top) for _ in range(3))
        assert pred(*t) == (t in acc), t
    # each dilation alone stays within the unit kernel's own range
    assert max(max(t) for t in acc) <= D_MAX[(C, k)]
    front = frontier(acc)
    picks = frontier_picks(front)
    assert all(p in acc for p in picks) and all(p in front for p in picks[:3])
    print("reschain C=%d k=%d: %d accepted triples, %d on the frontier, largest dilation %d, %d predicate calls, GPU picks %s"
          % (C, k, len(acc), len(front), top - 8, pred.calls, picks))


def test_reschain_refuses_outside_its_widths_and_taps(built_lib):
    arr = (ctypes.c_int * 3)(1, 3, 5)
    for C in WIDTHS:
        for k in range(14):
            want = int(C in (32, 64) and k in (3, 5, 7))
            assert built_lib.ctta_reschain_supported(C, k, arr) == want, (C, k)
    for bad in ((0, 3, 5), (1, 0, 5), (1, 3, -1)):
        assert built_lib.ctta_reschain_supported(32, 3, (ctypes.c_int * 3)(*bad)) == 0
    assert built_lib.ctta_reschain_supported(32, 3, None) == 0
