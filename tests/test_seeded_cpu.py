"""Seeded sampling, the halves that need no GPU: the numpy restatement of the stream (tests/philox_ref.py) against the
published known-answer vectors and against the standard normal, the two C entries in the header reader and in the built
library, every refusal of the C entries (raised before any launch: on this host a launch would be a HIP error, not an
argument error), and the ValueErrors of the Python surface, raised before anything touches a device."""
import ctypes
import math

import numpy as np
import pytest
import torch

import abi
import cases
import philox_ref as PR
from consistencytta_amd import _native as N
from consistencytta_amd.models import ConsistencyTTA

ENTRIES = ("ctta_philox_normal", "ctta_philox_words")


def test_restatement_reproduces_the_known_answer_vectors():
    for counter, key, want in PR.KNOWN_ANSWERS:
        got = tuple(int(v) for v in PR.philox4x32_10(counter, key))
        assert got == want, (["%08x" % v for v in got], ["%08x" % v for v in want])


def test_restatement_addresses_rows_as_the_outer_index():
    """q = (h * C + c) * W + w by hand on a (3, 5, 4) latent: one block per (h, c), block index h * 3 + c."""
    w = PR.words(1234, 2, 1, (3, 5, 4))
    for c, h in ((0, 0), (2, 0), (0, 1), (1, 4)):
        x = PR.philox4x32_10((h * 3 + c, 1, 2, 0), (1234, 0))
        assert [int(v) for v in x] == [int(v) for v in w[c, h]]
    hi = PR.words(-1, 0, 0, (3, 5, 4))                       # -1 is the key (0xffffffff, 0xffffffff)
    assert [int(v) for v in hi[0, 0]] == [int(v) for v in PR.philox4x32_10((0, 0, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF))]


def test_restatement_alone_is_standard_normal():
    """Conditions on the DEFINITION, not on the kernel: seed 1234, draw 0, sample 0, 32768 blocks = 131072 values.
    Measured for this input: |mean| 0.0037, |std - 1| 0.0023, KS distance 0.00275, max |z| 4.58."""
    _, z, _ = PR.normal([1234], None, 0, 1, (8, 1024, 16))
    z = np.sort(z.reshape(-1))
    n = z.size
    assert n == 131072
    mean, std, top = float(z.mean()), float(z.std()), float(np.abs(z).max())
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(z) / math.sqrt(2.0))).numpy()
    ks = float(max((np.arange(1, n + 1) / n - cdf).max(), (cdf - np.arange(0, n) / n).max()))
    print("restatement: mean %.4f std %.4f KS %.5f max|z| %.3f" % (mean, std, ks, top))
    assert abs(mean) <= 0.01
    assert abs(std - 1.0) <= 0.01
    assert ks <= 1.63 / math.sqrt(n) and 1.63 / math.sqrt(n) < 0.0046
    assert top <= 5.768 and abs(PR.MAX_ABS - 5.768) < 5e-4       # sqrt(-2 ln 2^-24) = 5.7681
    u = PR.unit(np.array([0, 0xFFFFFFFF], dtype=np.uint64))                  # strictly inside (0, 1), exact in fp32
    assert 0.0 < u[0] and u[1] < 1.0 and np.array_equal(u.astype(np.float32).astype(np.float64), u)


def test_entries_are_in_the_header_reader_and_in_the_built_library():
    for name in ENTRIES:
        assert name in N.FUNCTIONS
    abi.assert_bound(ENTRIES)
    f = N.FUNCTIONS["ctta_philox_normal"]
    assert f.c_argtypes == ["const int64_t*", "const int32_t*", "int", "int", "int", "int", "int", "int", "float", "float*",
                            "void*"]
    assert N.FUNCTIONS["ctta_philox_words"].c_argtypes == f.c_argtypes[:8] + ["int32_t*", "void*"]
    assert "philox" in open(N.CSRC + "/build.sh").read()


def test_entries_refuse_bad_arguments_before_any_launch():
    """Each refusal of include/ctta.h returns CTTA_ERR_INVALID -- the argument check's status; a launch attempted on this
    GPU-less host would come back as CTTA_ERR_HIP -- and leaves the output untouched."""
    L = abi.built_lib()
    invalid = N.CONSTANTS["CTTA_ERR_INVALID"]
    seeds = (ctypes.c_int64 * 4)(1, 2, 3, 4)
    out = (ctypes.c_float * 64)(*([7.0] * 64))
    good = dict(seeds=seeds, samples=None, batch=1, draw0=0, draws=1, channels=1, height=1, width=4, out=out)

    def call(**kw):
        a = dict(good, **kw)
        head = (a["seeds"], a["samples"], a["batch"], a["draw0"], a["draws"], a["channels"], a["height"], a["width"])
        return (L.ctta_philox_normal(*head, 1.0, a["out"], None), L.ctta_philox_words(*head, a["out"], None))

    bad = [dict(width=6), dict(width=2), dict(width=0), dict(width=-4), dict(batch=0), dict(batch=-1), dict(draws=0),
           dict(draws=-2), dict(channels=0), dict(height=0), dict(height=-8), dict(draw0=-1), dict(seeds=None),
           dict(out=None), dict(channels=1 << 10, height=1 << 20, width=1 << 4),             # C * H * W = 2^34
           dict(channels=(1 << 31) - 1, height=(1 << 31) - 1, width=(1 << 31) - 4)]           # far beyond 64 bits
    for kw in bad:
        assert call(**kw) == (invalid, invalid), kw
        assert L.ctta_last_error(), kw
    with pytest.raises(N.CttaError, match="multiple of 4"):
        N.check(call(width=6)[0])
    assert list(out) == [7.0] * 64


def _pipe():
    from consistencytta_amd import modules
    vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    return ConsistencyTTA(unet_config=cases.TINY_UNET, vae=vae).eval().requires_grad_(False)


def test_python_surface_refuses_a_wrong_seed_count_before_anything_runs():
    """Host module throughout: what passes the checks meets the missing CPU path (CttaError), never a launch.  The
    captured callables refuse through the loader `_serving_inputs` hands them, which is what is called here (a capture
    itself needs a GPU: tests/test_seeded_gpu.py calls the callables)."""
    pipe = _pipe()
    with pytest.raises(N.CttaError, match="no CPU path"):
        pipe.seeded_noise([1, 2], 2, (8, 32, 16))                  # everything in order: the checks pass
    with pytest.raises(N.CttaError, match="no CPU path"):
        pipe.seeded_noise(torch.tensor([1, 2]), 1, (8, 32, 16), samples=[0, 3], draw0=2)
    with pytest.raises(N.CttaError, match="no CPU path"):
        pipe.seeded_noise([2 ** 64 - 1, -2 ** 63], 1, (8, 32, 16))  # the whole uint64 range, and the whole int64 one
    for bad in ([], torch.zeros(0, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int64), torch.zeros(2), [2 ** 64], 7):
        with pytest.raises(ValueError, match="seeds"):
            pipe.seeded_noise(bad, 1, (8, 32, 16))
    with pytest.raises(ValueError, match="samples"):
        pipe.seeded_noise([1, 2], 1, (8, 32, 16), samples=[0])
    with pytest.raises(ValueError, match="samples"):
        pipe.seeded_noise([1, 2], 1, (8, 32, 16), samples=[0, -1])
    with pytest.raises(ValueError, match="num_draws"):
        pipe.seeded_noise([1], 0, (8, 32, 16))
    with pytest.raises(ValueError, match="draw0"):
        pipe.seeded_noise([1], 1, (8, 32, 16), draw0=-1)
    with pytest.raises(ValueError, match="latent"):
        pipe.seeded_noise([1], 1, (8, 32, 6))
    prompts = ["a dog barks", "rain"]
    wav = torch.zeros(2, 16000)
    for seeds in ([1], [1, 2, 3], [1, 2, 3, 4]):                   # 4 = the ROW count with num_samples 2: still one per prompt
        with pytest.raises(ValueError, match="seeds"):
            pipe.forward(prompts, num_steps=2, num_samples=2, seeds=seeds)
        with pytest.raises(ValueError, match="seeds"):
            pipe.generate_long(prompts, 5.0, num_samples=2, seeds=seeds)
        with pytest.raises(ValueError, match="seeds"):
            pipe.edit(prompts, wav, num_samples=2, seeds=seeds)
    B, Lx, D = 2, 5, cases.TINY_UNET["cross_attention_dim"]
    enc, mask = torch.zeros(B, Lx, D), torch.ones(B, Lx, dtype=torch.bool)
    st, load = pipe._serving_inputs(B, Lx, D, (8, 32, 16), 2, 1.0, None, None, False, seeded=True)
    assert st["seeds"].dtype == torch.int64 and st["samples"].dtype == torch.int32 and tuple(st["seeds"].shape) == (B,)
    load(enc, mask, [5, -6], samples=[1, 2])
    assert st["seeds"].tolist() == [5, -6] and st["samples"].tolist() == [1, 2]
    load(enc, mask, torch.tensor([2 ** 63 - 1, 0]))
    assert st["seeds"].tolist() == [2 ** 63 - 1, 0] and st["samples"].tolist() == [0, 0]
    for seeds in ([1], [1, 2, 3], torch.zeros(3, dtype=torch.int64), torch.zeros(2, 8, 32, 16)):
        with pytest.raises(ValueError, match="seeds"):
            load(enc, mask, seeds)
    with pytest.raises(ValueError, match="samples"):
        load(enc, mask, [1, 2], samples=[0, 1, 2])
    assert st["seeds"].tolist() == [2 ** 63 - 1, 0]                # a refused call changed nothing
    plain = pipe._serving_inputs(B, Lx, D, (8, 32, 16), 2, 1.0, None, None, False)
    assert "seeds" not in plain[0]
    with pytest.raises(TypeError):                                 # `samples=` belongs to the seeded form only
        plain[1](enc, mask, torch.zeros(2, B, 8, 32, 16), samples=[0, 0])
