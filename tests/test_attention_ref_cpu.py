"""The attention references against each other, on the CPU: the bf16 emulation of the kernels' arithmetic must itself
sit inside HALF of the forward bound on every case the GPU tests run, row by row -- otherwise a per-row bound derived
from it (tests/test_ops_gpu.py) would say nothing about the kernels."""
import math

import pytest
import torch

import attention_ref as R

HALF_BOUND = R.ROW_BOUND / 2


def _check(q, k, v, scale, bias, rel):
    ref, lse = R.attention_fp64(q, k, v, scale, bias, rel)
    emu = R.attention_bf16_emulated(q, k, v, scale, bias, rel)
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(emu).all())
    err = R.row_errors(emu, ref)
    worst = float(err.max())
    row_max = float(ref.abs().amax(dim=-1).min())
    print("worst row %.3e (limit %.3e), smallest row max of the reference %.3e" % (worst, HALF_BOUND, row_max))
    assert row_max > 1e-2          # no row so small that a relative error over it means nothing
    assert worst <= HALF_BOUND
    return ref, lse


@pytest.mark.parametrize("case", R.FWD_CASES)
def test_emulation_forward_cases(case):
    q, k, v, bias, scale = R.fwd_inputs(*case)
    _check(q, k, v, scale, bias, None)


@pytest.mark.parametrize("case", R.BWD_CASES_NEW)
def test_emulation_backward_cases_forward_half(case):
    B, heads, dh, nq, nk, _, _ = case
    q, k, v, bias, scale = R.fwd_inputs(B, heads, dh, nq, nk, False, prefix="fa")
    _check(q, k, v, scale, bias, None)


@pytest.mark.parametrize("case", R.REL_CASES)
def test_emulation_rel_cases(case):
    q, k, v, bias, rel, scale = R.rel_inputs(*case)
    _check(q, k, v, scale, bias, rel)


def test_emulation_rel_one_offset_case_and_what_an_index_slip_costs():
    B, heads, dh, nq, nk = R.REL_ONE_OFFSET_CASE
    q, k, v, bias, rel, scale = R.rel_inputs(B, heads, dh, nq, nk, one_offset=True)
    ref, _ = _check(q, k, v, scale, bias, rel)
    # the case is only worth running if a table read one entry off is far outside the bound, not a shifted norm
    for shift in (-1, 1):
        slipped, _ = R.attention_fp64(q, k, v, scale, bias, torch.roll(rel, shift, dims=1))
        assert float(R.row_errors(slipped, ref).max()) > 0.5


def test_fp64_reference_is_the_plain_formula():
    """attention_fp64 against an independent element-by-element evaluation, with a bias and a table."""
    B, heads, dh, nq, nk = 2, 2, 5, 6, 4
    q, k, v, bias, rel, _ = R.rel_inputs(B, heads, dh, nq, nk)
    scale = 0.37
    ref, lse = R.attention_fp64(q, k, v, scale, bias, rel)
    for b in range(B):
        for h in range(heads):
            for i in range(nq):
                s = [sum(float(q[b, h, i, d]) * float(k[b, h, j, d]) for d in range(dh)) * scale + float(bias[b, j]) +
                     float(rel[h, j - i + nq - 1]) for j in range(nk)]
                m = max(s)
                e = [math.exp(x - m) for x in s]
                z = sum(e)
                assert abs((m + math.log(z)) * R.LOG2E - float(lse[b, h, i])) < 1e-9
                for d in range(dh):
                    want = sum(e[j] / z * float(v[b, h, j, d]) for j in range(nk))
                    assert abs(want - float(ref[b, h, i, d])) < 1e-12
