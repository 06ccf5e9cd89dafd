"""Host side of the VAE decoder's parameter-gradient operators: the header, the ctypes table and the library agree on the
new entries, the implicit kernel's range grew by width 64 and by nothing else, and the scratch sizes are what the launchers
use."""
import os

import pytest

import abi
from consistencytta_amd import _native as N

NEW = ("ctta_conv_cout1_wgrad", "ctta_conv_cout1_wgrad_scratch_floats", "ctta_post_quant_wgrad",
       "ctta_post_quant_wgrad_scratch_floats", "ctta_upsample2_nearest")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def test_header_signatures_and_library_agree_on_the_new_entries(L):
    abi.assert_bound(NEW, L)


def test_implicit_range_grew_by_width_64_only(L):
    sup = L.ctta_wgrad_implicit_supported
    for c, h, n in ((32, 1, 8), (40, 2, 72), (64, 3, 64), (128, 1024, 128), (256, 1024, 128)):
        assert sup(9, c, h, 64, c, n) == 1
    # the c, x_ld and n rules hold at the new width too
    assert sup(9, 24, 8, 64, 24, 64) == 0 and sup(9, 36, 8, 64, 36, 64) == 0 and sup(9, 64, 8, 64, 68, 64) == 0
    assert sup(9, 64, 8, 64, 64, 4) == 0
    # every other width answers as before: powers of two from 2 to 32 with h * w a multiple of 64
    for w in range(1, 200):
        if w == 64:
            continue
        for h in (1, 2, 6, 8, 32, 64):
            want = 1 if (2 <= w <= 32 and w & (w - 1) == 0 and (h * w) % 64 == 0) else 0
            assert sup(9, 64, h, w, 64, 64) == want, (h, w)
    assert sup(1, 64, 7, 5, 64, 64) == 1 and sup(4, 64, 8, 8, 64, 64) == 0


def test_scratch_sizes(L):
    # one partial row of c * taps + 1 floats per workgroup; a workgroup per 16 pixels of each of its 256 / (c / 8) phases
    assert L.ctta_conv_cout1_wgrad_scratch_floats(2, 4, 8, 3, 3, 32) == 9 * 32 + 1
    assert L.ctta_conv_cout1_wgrad_scratch_floats(2, 8, 64, 3, 3, 128) == 4 * (9 * 128 + 1)
    assert L.ctta_conv_cout1_wgrad_scratch_floats(4, 1024, 64, 3, 3, 128) == 512 * (9 * 128 + 1)
    assert L.ctta_conv_cout1_wgrad_scratch_floats(1, 4, 4, 3, 3, 12) == 0         # outside the kernel's range
    assert L.ctta_post_quant_wgrad_scratch_floats(2, 16, 8, 8) == 72
    assert L.ctta_post_quant_wgrad_scratch_floats(3, 100, 8, 8) == 3 * 72
    assert L.ctta_post_quant_wgrad_scratch_floats(4, 4096, 8, 8) == 128 * 72
    assert L.ctta_post_quant_wgrad_scratch_floats(1, 16, 17, 8) == 0
