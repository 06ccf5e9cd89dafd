"""The per-sample adapter kernels (csrc/lora.hip: ctta_lora_down_rows / _up_add_rows / _up_add_t_rows) through the C ABI.

Two references.  (1) The per-site kernels they extend, launched once per sample on that sample's rows with that slot's
matrix and that scale: the rows kernels must give the same BITS (`torch.equal`), and rows whose slot is outside the bank
keep y's bits and get d = 0.  (2) float64 torch on the same bf16-rounded inputs, under the per-element bounds of
test_lora_ops_gpu.py (restated from its docstring; fp32 accumulation, u = 2^-24, one bf16 rounding asserted as 2^-8):
  down    |got - ref| <= K u sum|x a|
  up_add  |got - ref| <= 2^-8 |ref| + r u sum|terms|

Batch 5 over a bank of 3 slots, slots [2, -1, 0, 2, 7] (-1: the base model, 7: too large), slot 1 never loaded (zeros).
The shapes reach every branch: the four lanes-per-row forms (k 64 / 128 / 256 / 320), both rank instantiations (r <= 4, r > 4),
samples inside one wave (8 rows), blocks that would straddle samples (24), aligned (64) and several blocks with a tail (200).
"""
import pytest
import torch

from consistencytta_amd import _native as N
from gpu_util import DEV, bf16_round, det, sync

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
RANKS = (1, 4, 5, 16)
RPS = (8, 24, 64, 200)
BATCH, N_SLOTS = 5, 3
SLOTS = [2, -1, 0, 2, 7]
SCALES = [1.0, 3.0, 0.5, 0.0, 1.0]
GUARD = 4            # rows behind the last one that no launch may touch
ARG_SCALE = 0.75     # the `scale` argument: every row's strength when the array is NULL, ignored when it is given


def valid(s):
    return 0 <= s < N_SLOTS


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def dev_rows():
    return torch.tensor(SLOTS, dtype=torch.int32, device=DEV), torch.tensor(SCALES, dtype=torch.float32, device=DEV)


def bank_of(name, shape, scale=0.5):
    """(N_SLOTS, *shape) fp32: slots 0 and 2 loaded, slot 1 all zeros (never loaded)"""
    b = torch.stack([det("%s.%d" % (name, s), shape, scale=scale) for s in range(N_SLOTS)])
    b[1] = 0
    return b


@pytest.mark.parametrize("k", [64, 128, 256, 320])
def test_down_rows(k):
    L = N.lib()
    slot_dev, _ = dev_rows()
    for r in RANKS:
        bank = bank_of("rows.down.a.%d.%d" % (k, r), (r, k))
        bank_dev = bank.to(DEV)
        for rps in RPS:
            m = BATCH * rps
            xl = bf16_round(det("rows.down.x.%d.%d" % (k, rps), (m, k)))
            x = xl.to(torch.bfloat16).to(DEV)
            d = torch.full((m + GUARD, r), float("nan"), device=DEV)
            N.check(L.ctta_lora_down_rows(N.ptr(x), k, m, k, N.ptr(bank_dev), r * k, N_SLOTS, r, rps, N.ptr(slot_dev), N.ptr(d),
                                          N.stream_ptr()))
            want = torch.zeros(m, r, device=DEV)
            for b, s in enumerate(SLOTS):
                if valid(s):
                    N.check(L.ctta_lora_down(N.ptr(x[b * rps:]), k, rps, k, N.ptr(bank_dev[s]), 0, r, N.ptr(want[b * rps:]),
                                             N.stream_ptr()))
            sync()
            assert torch.equal(bits(d[:m]), bits(want)), (k, r, rps)
            assert bool(torch.isnan(d[m:]).all()), "the guard rows behind d were written"
            got = d[:m].cpu().double()
            for b, s in enumerate(SLOTS):
                rows = slice(b * rps, (b + 1) * rps)
                if not valid(s):
                    assert float(got[rows].abs().max()) == 0.0, (k, r, rps, b)
                    continue
                ref = xl[rows].double() @ bank[s].double().t()
                bound = k * U * (xl[rows].double().abs() @ bank[s].double().abs().t()) + 1e-30
                err = (got[rows] - ref).abs()
                assert bool((err <= bound).all()), (k, r, rps, b, float((err / bound).max()))
                assert float(got[rows].abs().max()) > 0.0


@pytest.mark.parametrize("with_scales", [True, False], ids=["scale_array", "scale_null"])
@pytest.mark.parametrize("n", [64, 320])
def test_up_add_rows(n, with_scales):
    L = N.lib()
    slot_dev, scale_dev = dev_rows()
    zero_slot = torch.ones(BATCH, dtype=torch.int32, device=DEV)          # every row asks for the never-loaded slot
    for r in RANKS:
        bank = bank_of("rows.up.b.%d.%d" % (n, r), (n, r))
        bank_dev = bank.to(DEV)
        for rps in RPS:
            m = BATCH * rps
            dd = det("rows.up.d.%d.%d" % (r, rps), (m, r))
            dd_dev = dd.to(DEV)
            yl = bf16_round(det("rows.up.y.%d.%d" % (n, rps), (m + GUARD, n)))
            y0 = yl.to(torch.bfloat16).to(DEV)
            y = y0.clone()
            # with the array given the scale argument must be ignored (it is not a factor): hand over a large one
            N.check(L.ctta_lora_up_add_rows(N.ptr(y), n, m, n, N.ptr(dd_dev), N.ptr(bank_dev), n * r, N_SLOTS, r, rps,
                                            N.ptr(slot_dev), N.ptr(scale_dev) if with_scales else None,
                                            1000.0 if with_scales else ARG_SCALE, N.stream_ptr()))
            want = y0.clone()
            for b, s in enumerate(SLOTS):
                if valid(s):
                    N.check(L.ctta_lora_up_add(N.ptr(want[b * rps:]), n, rps, n, N.ptr(dd_dev[b * rps:]), N.ptr(bank_dev[s]), 0, r,
                                               SCALES[b] if with_scales else ARG_SCALE, N.stream_ptr()))
            z = y0.clone()
            N.check(L.ctta_lora_up_add_rows(N.ptr(z), n, m, n, N.ptr(dd_dev), N.ptr(bank_dev), n * r, N_SLOTS, r, rps,
                                            N.ptr(zero_slot), None, 1.0, N.stream_ptr()))
            sync()
            assert torch.equal(bits(y), bits(want)), (n, r, rps)          # guard rows included
            assert torch.equal(bits(y[m:]), bits(y0[m:])), "the guard rows behind y were written"
            assert torch.equal(bits(z), bits(y0)), "a never-loaded (all-zero) slot changed y"
            got = y.float().cpu().double()
            for b, s in enumerate(SLOTS):
                rows = slice(b * rps, (b + 1) * rps)
                scale = SCALES[b] if with_scales else ARG_SCALE
                if not valid(s) or scale == 0.0:
                    assert torch.equal(bits(y[rows]), bits(y0[rows])), (n, r, rps, b)
                    continue
                terms = scale * dd[rows].double()[:, None, :] * bank[s].double()[None, :, :]
                ref = yl[rows].double() + terms.sum(-1)
                bound = 2.0 ** -8 * ref.abs() + r * U * terms.abs().sum(-1) + 1e-30
                err = (got[rows] - ref).abs()
                assert bool((err <= bound).all()), (n, r, rps, b, float((err / bound).max()))
                assert not torch.equal(bits(y[rows]), bits(y0[rows]))


@pytest.mark.parametrize("with_scales", [True, False], ids=["scale_array", "scale_null"])
@pytest.mark.parametrize("tokens,d_tokens", [(8, 16), (5, 9)], ids=["vector", "scalar"])
def test_up_add_t_rows(tokens, d_tokens, with_scales):
    L = N.lib()
    slot_dev, scale_dev = dev_rows()
    zero_slot = torch.ones(BATCH, dtype=torch.int32, device=DEV)
    ldt = 8
    for n in (64, 320):
        for r in RANKS:
            bank = bank_of("rows.upt.b.%d.%d" % (n, r), (n, r))
            bank_dev = bank.to(DEV)
            dd = det("rows.upt.d.%d.%d" % (r, d_tokens), (BATCH * d_tokens, r))
            dd_dev = dd.to(DEV)
            yl = bf16_round(det("rows.upt.y.%d.%d" % (n, tokens), (BATCH + 1, n, ldt)))      # one guard sample behind
            y0 = yl.to(torch.bfloat16).to(DEV)
            y = y0.clone()
            N.check(L.ctta_lora_up_add_t_rows(N.ptr(y), ldt, n * ldt, BATCH, tokens, n, N.ptr(dd_dev), d_tokens, N.ptr(bank_dev),
                                              n * r, N_SLOTS, r, N.ptr(slot_dev), N.ptr(scale_dev) if with_scales else None,
                                              1000.0 if with_scales else ARG_SCALE, N.stream_ptr()))
            want = y0.clone()
            for b, s in enumerate(SLOTS):
                if valid(s):
                    N.check(L.ctta_lora_up_add_t(N.ptr(want[b]), ldt, n * ldt, 1, tokens, n, N.ptr(dd_dev[b * d_tokens:]), d_tokens,
                                                 N.ptr(bank_dev[s]), r, SCALES[b] if with_scales else ARG_SCALE, N.stream_ptr()))
            z = y0.clone()
            N.check(L.ctta_lora_up_add_t_rows(N.ptr(z), ldt, n * ldt, BATCH, tokens, n, N.ptr(dd_dev), d_tokens, N.ptr(bank_dev),
                                              n * r, N_SLOTS, r, N.ptr(zero_slot), None, 1.0, N.stream_ptr()))
            sync()
            assert torch.equal(bits(y), bits(want)), (n, r, tokens)
            assert torch.equal(bits(y[BATCH]), bits(y0[BATCH])), "the guard sample behind yt was written"
            assert torch.equal(bits(y[:, :, tokens:]), bits(y0[:, :, tokens:])), "columns behind the tokens were written"
            assert torch.equal(bits(z), bits(y0)), "a never-loaded (all-zero) slot changed yt"
            got = y.float().cpu().double()
            for b, s in enumerate(SLOTS):
                scale = SCALES[b] if with_scales else ARG_SCALE
                if not valid(s) or scale == 0.0:
                    assert torch.equal(bits(y[b]), bits(y0[b])), (n, r, tokens, b)
                    continue
                drow = dd[b * d_tokens:b * d_tokens + tokens].double()                         # (tokens, r)
                terms = scale * drow[None, :, :] * bank[s].double()[:, None, :]                # (n, tokens, r)
                ref = yl[b, :, :tokens].double() + terms.sum(-1)
                bound = 2.0 ** -8 * ref.abs() + r * U * terms.abs().sum(-1) + 1e-30
                err = (got[b, :, :tokens] - ref).abs()
                assert bool((err <= bound).all()), (n, r, tokens, b, float((err / bound).max()))
                assert not torch.equal(bits(y[b]), bits(y0[b]))


def test_bad_arguments_are_refused():
    L = N.lib()
    t = torch.zeros(64, 64, dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(3 * 64 * 4, device=DEV)
    s = torch.zeros(8, dtype=torch.int32, device=DEV)
    sp = N.stream_ptr()
    assert L.ctta_lora_down_rows(N.ptr(t), 64, 8, 64, N.ptr(f), 4 * 64, 3, 4, 8, None, N.ptr(f), sp) != 0          # no slot array
    assert L.ctta_lora_down_rows(N.ptr(t), 64, 8, 64, N.ptr(f), 4 * 64, 0, 4, 8, N.ptr(s), N.ptr(f), sp) != 0      # no slots
    assert L.ctta_lora_down_rows(N.ptr(t), 64, 8, 64, N.ptr(f), 4 * 64 - 4, 3, 4, 8, N.ptr(s), N.ptr(f), sp) != 0  # slots overlap
    assert L.ctta_lora_down_rows(N.ptr(t), 64, 8, 64, N.ptr(f), 4 * 64, 3, 17, 8, N.ptr(s), N.ptr(f), sp) != 0     # rank
    assert L.ctta_lora_up_add_rows(N.ptr(t), 64, 8, 64, N.ptr(f), N.ptr(f), 64 * 4, 3, 4, 0, N.ptr(s), None, 1.0, sp) != 0   # rows per sample
    assert L.ctta_lora_up_add_t_rows(N.ptr(t), 8, 64 * 8, 1, 8, 64, N.ptr(f), 4, N.ptr(f), 64 * 4, 3, 4, N.ptr(s), None, 1.0, sp) != 0
