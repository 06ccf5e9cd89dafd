"""The accepted region of the fused HiFi-GAN ResBlock kernels (csrc/resunit.hip), written out by hand for the tests.

ctta_resunit_supported(C, k, d) and ctta_reschain_supported(C, k, dils) are the contract of the two kernels: a shape they
accept must be computed correctly.  This module holds what the tests pin that contract to -- the largest dilation per
(C, k), the tile the launcher picks, the LDS arithmetic and the per-sample extent limit, each mirrored from the kernel's
own expressions -- and the walk that enumerates every accepted dilation triple of the chained kernel.
"""
import ctypes

LDS_SMALL = 64 * 1024           # C <= 128: three workgroups per CU
LDS_BIG = 160 * 1024            # C = 256 / 512: one workgroup per CU
ANY = float("inf")              # k = 1: the dilation never reaches the kernel (no halo)

# Largest accepted dilation per (C, k).  Pairs not listed are refused whatever d is: even k, C outside
# {32, 64, 128, 256, 512}, and C = 512 with k in {1, 5, 9}.
D_MAX = {
    (32, 1): ANY, (32, 3): 121, (32, 5): 60, (32, 7): 40, (32, 9): 30, (32, 11): 24,
    (64, 1): ANY, (64, 3): 83, (64, 5): 41, (64, 7): 27, (64, 9): 20, (64, 11): 16,
    (128, 1): ANY, (128, 3): 48, (128, 5): 24, (128, 7): 16, (128, 9): 12, (128, 11): 9,
    (256, 1): ANY, (256, 3): 51, (256, 5): 17, (256, 7): 11, (256, 9): 8, (256, 11): 7,
    (512, 3): 38, (512, 7): 10, (512, 11): 6,
}
# C = 512: the first dilation that no longer fits the 96-position tile (k = 3 then takes 64 positions, k = 7 / 11 take 80)
TILE_SWITCH_512 = {3: 23, 7: 8, 11: 5}


def halo1(k, d):
    return d * (k - 1) // 2


def resunit_geom(C, k, d):
    """(T, WP, NT) of the launcher: positions per workgroup, wave parts, threads per workgroup."""
    if C == 512:
        return (96 if d < TILE_SWITCH_512[k] else 64 if k == 3 else 80), 1, 512
    if C == 256:
        return (192 if k <= 3 else 224), 1, 512
    return {128: (128, 1, 256), 64: (256, 2, 256), 32: (512, 4, 256)}[C]


def resunit_lds(C, WP, T, k, d):
    """Bytes of LDS resunit_kernel needs: the staged rows (T/16/WP + 1 blocks of 16 per wave part plus the conv1 halo on both
    sides, C + 8 bf16 per row), or the epilogue's fp32 transpose (32 rows per part, 4C + 16 bytes per row) if larger."""
    return max((T + 16 * WP + 2 * halo1(k, d)) * (C + 8) * 2, WP * 32 * (4 * C + 16))


def resunit_fits(C, k, d):
    T, WP, _ = resunit_geom(C, k, d)
    return resunit_lds(C, WP, T, k, d) <= (LDS_BIG if C >= 256 else LDS_SMALL)


def resunit_max_len(C, k, d):
    """Longest sequence ctta_resunit_conv1d accepts.  The last tile (first position l0) stages rows
    l0 - H1 - H2 + [0, (R // BR + 1) * BR): R = T + 16 WP + 2 H1 rows in load batches of BR = 4 NT / (C / 8) rows, the last
    batch loaded whole.  Its signed 32-bit byte offsets stay below 2^31 while those rows times 2C bytes are <= 2^31."""
    T, WP, NT = resunit_geom(C, k, d)
    h1, h2 = halo1(k, d), (k - 1) // 2
    br = 4 * NT // (C // 8)
    past_l0 = ((T + 16 * WP + 2 * h1) // br + 1) * br - h1 - h2
    return ((1 << 30) // C - past_l0) // T * T + T


RESCHAIN_TILE = {32: 256, 64: 128}


def reschain_max_len(C):
    """Longest sequence ctta_reschain_conv1d accepts: the epilogue stores up to row ceil(L / T) * T of a sample with signed
    32-bit byte offsets (it stages through 64-bit pointers)."""
    T = RESCHAIN_TILE[C]
    return (1 << 30) // C // T * T


def reschain_halo(k, dils):
    return sum((d + 1) * ((k - 1) // 2) for d in dils)


class ChainPredicate:
    """ctta_reschain_supported with one reused argument array (the walk makes ~10^5 calls)."""

    def __init__(self, lib, C, k):
        self.fn, self.C, self.k = lib.ctta_reschain_supported, C, k
        self.arr = (ctypes.c_int * 3)()
        self.calls = 0

    def __call__(self, d0, d1, d2):
        self.arr[0], self.arr[1], self.arr[2] = d0, d1, d2
        self.calls += 1
        return self.fn(self.C, self.k, self.arr) == 1


def reschain_accepted(pred):
    """Every accepted triple reachable from (1, 1, 1): raise d2 until refused, then the next d1, then the next d0.  Exhaustive
    when the accepted set is downward-closed (checked by the tests)."""
    acc = set()
    d0 = 1
    while pred(d0, 1, 1):
        d1 = 1
        while pred(d0, d1, 1):
            d2 = 1
            while pred(d0, d1, d2):
                acc.add((d0, d1, d2))
                d2 += 1
            d1 += 1
        d0 += 1
    return acc


def raised(t):
    return [t[:i] + (t[i] + 1,) + t[i + 1:] for i in range(3)]


def frontier(acc):
    """Accepted triples where raising any one dilation leaves the accepted set."""
    return sorted(t for t in acc if all(r not in acc for r in raised(t)))


def frontier_picks(front):
    """The chained GPU cases of one (C, k): the frontier triple with the largest d0, the one with the largest d2, the most
    balanced one (largest smallest dilation), and HiFi-GAN's own (1, 3, 5)."""
    return [max(front, key=lambda t: (t[0], t[1] + t[2], t)), max(front, key=lambda t: (t[2], t[0] + t[1], t)),
            max(front, key=lambda t: (min(t), sum(t), t)), (1, 3, 5)]
