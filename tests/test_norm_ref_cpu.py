"""tests/norm_ref.py checked on the CPU: the float64 closed-form backwards against torch.autograd, the input generators against
what they promise, the fp32 emulation of GroupNorm's statistics against the bounds (the reference side alone must stay well
inside them, or a kernel could not), and the case tables against the dispatchers' predicates: every form is reached."""
import math

import pytest
import torch
import torch.nn.functional as F

import norm_ref as R


# ------------------------------------------------------------------------------------------------ closed forms vs autograd
@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_closed_form_backward_equals_autograd(silu):
    B, C, hw, G = 2, 24, 15, 3
    x = R.gn_input("benign", B, C, hw, G, "cpu.gn").double().requires_grad_(True)
    gamma, beta = [t.double().requires_grad_(True) for t in R.affine(C, "cpu.gn")]
    dy = R.bf16_round(R.det("cpu.gn.dy", (B, hw, C), 4)).double()
    y = F.group_norm(x.permute(0, 2, 1), G, gamma, beta, R.f32(R.GN_EPS)).permute(0, 2, 1)
    if silu:
        y = F.silu(y)
    y.backward(dy)
    yr, mean, rstd = R.gn_forward_ref(x.detach(), G, gamma.detach(), beta.detach(), R.GN_EPS, silu)
    assert float((yr - y.detach()).abs().max()) < 1e-10
    dx, dg, db, ag, ab = R.gn_backward_ref(x.detach(), dy, G, gamma.detach(), beta.detach(), R.GN_EPS, silu)
    assert float((dx - x.grad).abs().max()) < 1e-10
    assert float((dg - gamma.grad).abs().max()) < 1e-10 and float((db - beta.grad).abs().max()) < 1e-10
    assert bool((ag >= dg.abs()).all()) and bool((ab >= db.abs()).all())
    # the same closed form from statistics it is handed
    dx2, dg2, _, _, _ = R.gn_backward_ref(x.detach(), dy, G, gamma.detach(), beta.detach(), R.GN_EPS, silu,
                                          stats=torch.stack([mean, rstd], dim=-1))
    assert float((dx2 - dx).abs().max()) < 1e-12 and float((dg2 - dg).abs().max()) < 1e-12
    assert float((R.gn_apply_ref(x.detach(), G, gamma.detach(), beta.detach(), mean, rstd, silu) - yr).abs().max()) < 1e-12


def test_layernorm_closed_form_backward_equals_autograd():
    rows, d, ld = 7, 21, 24
    xp = R.rows_input("benign", rows, d, ld, "cpu.ln")
    x = xp[:, :d].double().requires_grad_(True)
    gamma, beta = [t.double().requires_grad_(True) for t in R.affine(d, "cpu.ln")]
    dyp = R.bf16_round(R.det("cpu.ln.dy", (rows, ld), 4))
    y = F.layer_norm(x, (d,), gamma, beta, R.f32(R.LN_EPS))
    y.backward(dyp[:, :d].double())
    yr = R.ln_forward_ref(xp, d, gamma.detach(), beta.detach(), R.LN_EPS)
    assert float((yr[:, :d] - y.detach()).abs().max()) < 1e-10 and float(yr[:, d:].abs().max()) == 0.0
    dx, dg, db, ag, ab = R.ln_backward_ref(xp, dyp, d, gamma.detach(), R.LN_EPS)
    assert float((dx[:, :d] - x.grad).abs().max()) < 1e-10 and float(dx[:, d:].abs().max()) == 0.0
    assert float((dg - gamma.grad).abs().max()) < 1e-10 and float((db - beta.grad).abs().max()) < 1e-10
    assert bool((ag >= dg.abs()).all()) and bool((ab >= db.abs()).all())


def test_softmax_closed_form_backward_equals_autograd():
    rows, cols, lds, rpb, scale = 6, 19, 24, 3, 0.14
    sp = R.softmax_scores("benign", rows, cols, lds, scale, "cpu.sm")
    s = sp[:, :cols].double().requires_grad_(True)
    bias = R.softmax_bias("mask_tail", rows // rpb, cols)
    p = torch.softmax(s * R.f32(scale) + bias.double().repeat_interleave(rpb, 0), dim=-1)
    dp = R.det("cpu.sm.dp", (rows, cols), 2)
    p.backward(dp.double())
    pr = R.softmax_ref(sp, cols, scale, bias, rpb)
    assert float((pr - p.detach()).abs().max()) < 1e-10
    ds, dot_abs = R.softmax_backward_ref(pr, dp, cols, scale)
    assert float((ds - s.grad).abs().max()) < 1e-10
    assert bool((dot_abs.view(-1) >= (pr * dp.double()).sum(1).abs()).all())


# ------------------------------------------------------------------------------------------------ generators
@pytest.mark.parametrize("kind,ratio", [("offset16", 16.0), ("offset64", 64.0)])
def test_offset_inputs_have_the_requested_mean_to_std_ratio_after_bf16_rounding(kind, ratio):
    B, C, hw, G = 2, 40, 45, 8                                   # the smallest slab of the tables
    x = R.gn_input(kind, B, C, hw, G, "cpu.gen")
    assert torch.equal(x, R.bf16_round(x))
    xs = x.double().view(B, hw, G, C // G)
    r = xs.mean(dim=(1, 3)).abs() / xs.var(dim=(1, 3), unbiased=False).sqrt()
    assert float((r / ratio - 1).abs().max()) < 0.10, r
    assert float(xs.mean(dim=(1, 3)).min()) < 0 < float(xs.mean(dim=(1, 3)).max())       # both signs occur
    xr = R.rows_input(kind, 9, 96, 104, "cpu.gen")[:, :96].double()
    rr = xr.mean(1).abs() / xr.var(1, unbiased=False).sqrt()
    assert float((rr / ratio - 1).abs().max()) < 0.10, rr


def test_constant_inputs_have_exactly_zero_variance_and_benign_neighbours():
    B, C, hw, G = 2, 40, 45, 8
    xs = R.gn_input("constant", B, C, hw, G, "cpu.gen").double().view(B, hw, G, C // G)
    var = xs.var(dim=(1, 3), unbiased=False)
    for b in range(B):
        for g in range(G):
            assert (float(var[b, g]) == 0.0) == R.constant_slab(b, g)
    xr = R.rows_input("constant", 9, 96, 104, "cpu.gen")
    v = xr[:, :96].double().var(1, unbiased=False)
    assert all((float(v[r]) == 0.0) == (r % 2 == 0) for r in range(9))
    assert bool((xr[:, 96:] == 7.0).all())                        # the pad columns carry a value the kernels must ignore


def test_softmax_inputs_are_as_hostile_as_they_say():
    rows, cols, scale = 5, 36, 0.044
    for lds in (cols, cols + 4):
        eq = R.softmax_scores("equal", rows, cols, lds, scale, "cpu.gen")[:, :cols]
        assert bool((eq == eq[:, :1]).all())
        sp = R.softmax_scores("spike60", rows, cols, lds, scale, "cpu.gen")[:, :cols].double() * R.f32(scale)
        top = sp.topk(2, dim=1).values
        assert float((top[:, 0] - top[:, 1]).min()) >= 60.0 - 1e-3
        sn = R.softmax_scores("span80", rows, cols, lds, scale, "cpu.gen")[:, :cols].double() * R.f32(scale)
        assert abs(float(sn.max()) - 80.0) < 1e-3 and abs(float(sn.min()) + 80.0) < 1e-3
    ball, bone = R.softmax_bias("mask_all", 4, cols), R.softmax_bias("mask_but_one", 4, cols)
    assert bool((ball[1] == -10000.0).all()) and int((bone[3] == 0).sum()) == 1 and int((bone[3] == -10000.0).sum()) == cols - 1
    # a fully masked row is still a distribution, and the survivor of mask_but_one takes all of it
    p = R.softmax_ref(R.softmax_scores("benign", 4, cols, cols, scale, "cpu.gen"), cols, scale, bone, 1)
    assert float(p[3].max()) == 1.0


# ------------------------------------------------------------------------------------------------ the emulation vs the bounds
def _emulation_loss(case, kind):
    B, C, hw, G, _ = case
    x = R.gn_input(kind, B, C, hw, G, "fwd.%d.%d.%d.%d" % (B, C, hw, G))[:1]          # sample 0: a slab never sees its batch
    gamma, beta = R.affine(C, "fwd")
    em_mean, em_rstd = R.gn_stats_emulated(x, G)
    _, mean, rstd = R.gn_forward_ref(x, G, gamma, beta, R.GN_EPS, False)
    bm, br = R.stats_bounds(mean, rstd)
    r_mean = R.worst_ratio((em_mean.double() - mean).abs(), bm)
    r_rstd = R.worst_ratio((em_rstd.double() - rstd).abs(), br)
    worst_fwd = 0.0
    for silu in (False, True):
        ref = R.gn_apply_ref(x, G, gamma, beta, mean, rstd, silu)
        em = R.gn_apply_ref(x, G, gamma, beta, em_mean, em_rstd, silu)
        worst_fwd = max(worst_fwd, R.worst_ratio((em - ref).abs(), R.fwd_bound(ref, R.slab_max(ref, G))))
    rel_rstd = float(((em_rstd.double() - rstd).abs() / rstd).max())
    return r_mean, r_rstd, worst_fwd, rel_rstd


@pytest.mark.parametrize("case", R.GN_FWD_CASES, ids=lambda c: "B%d-C%d-hw%d-G%d" % c[:4])
def test_emulated_statistics_stay_inside_a_quarter_of_the_bounds(case):
    line = "%2d %4d %4d %2d |" % case[:4]
    for kind in ("benign", "offset16", "offset64"):
        r_mean, r_rstd, r_fwd, rel_rstd = _emulation_loss(case, kind)
        line += "  %.1e / %.3f  |" % (rel_rstd, r_mean)
        assert r_mean <= 0.25 and r_rstd <= 0.25 and r_fwd <= 0.25, (kind, r_mean, r_rstd, r_fwd)
    print(line)


def test_emulation_forms_agree_on_an_exact_input():
    """Small integers sum exactly in fp32 in any order: both emulated forms must give the float64 statistics to fp32 rounding."""
    B, C, hw, G = 1, 64, 40, 4
    x = torch.round(R.det("cpu.em", (B, hw, C), 1) * 4)
    _, mean, rstd = R.gn_forward_ref(x, G, torch.ones(C), torch.zeros(C), R.GN_EPS, False)
    for form in ("small", "chunked"):
        m, r = R.gn_stats_emulated(x, G, form=form)
        assert torch.equal(m, mean.float()) and torch.equal(r, rstd.float())


# ------------------------------------------------------------------------------------------------ the tables reach every form
def test_groupnorm_forward_table_reaches_every_form():
    seen = set()
    for B, C, hw, G, form in R.GN_FWD_CASES:
        forms = R.gn_fwd_forms(B, C, hw, G)
        assert form in forms, (B, C, hw, G, form, forms)
        assert B * hw * C * 2 < 10e6
        seen |= forms
    assert seen == R.GN_FWD_FORMS
    # what the table's comments promise
    assert R.gn_small_ok(2048, 256, 32) and 2048 * (256 // 32) // 8 == 8 * 256 and not R.gn_small_ok(2049, 256, 32)
    assert R.gn_geometry(1031, 2048) == (16, 65) and 1031 % 16 != 0 and 65 * 32 > 2048
    assert R.gn_finalize_lanes(24) == 1 and R.gn_finalize_lanes(1) == 64 and R.gn_finalize_lanes(32) == 8


def test_groupnorm_from_partials_table_reaches_every_form():
    seen = set()
    for B, C1, C2, hw, G, stats, form in R.GN_PARTIALS_CASES:
        C = C1 + C2
        assert not R.gn_small_ok(hw, C, G)            # ctta_groupnorm takes the same chunking: the bit-identity holds
        assert R.gn_partials_form(C, G, R.gn_geometry(hw, C)[1], stats) == form
        assert B * hw * C * 2 < 10e6
        seen.add(form)
    assert seen == R.GN_PARTIALS_FORMS
    assert (328 // (640 // 32)) * (640 // 32) != 328          # a group straddles the two sources


def test_layernorm_forward_table_reaches_every_form():
    seen = set()
    for rows, d, ld, form in R.LN_FWD_CASES:
        assert R.ln_fwd_form(ld) == form and d <= ld and ld % 8 == 0
        seen.add(form)
    assert seen == R.LN_FWD_FORMS
    for rows, d, ld, form in R.LN_FWD_CASES:
        if form.startswith("fast"):
            assert rows % R.ln_fwd_rows_per_block(ld) != 0 and rows > R.ln_fwd_rows_per_block(ld)
    assert any(d < ld for _, d, ld, f in R.LN_FWD_CASES if f == "rows<64>")


def test_softmax_table_reaches_every_form():
    assert {R.softmax_form(c) for _, c, _ in R.SOFTMAX_CASES} == R.SOFTMAX_FORMS
    assert all(R.softmax_form(c) == f and c % 4 == 0 for _, c, f in R.SOFTMAX_CASES)
    generic = [c for _, c, f in R.SOFTMAX_CASES if f == "generic"]
    assert any(c > 1024 and c % 1024 for c in generic) and any(c < 1024 for c in generic)      # a partial last trip
    for rows, cols, ldp, rpb, lds, with_bias in R.SOFTMAX_BIAS_CASES:
        assert ldp >= cols and lds >= cols and rows % rpb == 0
    assert any(c[1] > 256 for c in R.SOFTMAX_BIAS_CASES) and any(c[1] > 1024 for c in R.SOFTMAX_BIAS_CASES)
    assert any(c[4] > c[1] for c in R.SOFTMAX_BIAS_CASES) and any(not c[5] for c in R.SOFTMAX_BIAS_CASES)


def test_groupnorm_backward_table_reaches_every_form():
    seen = set()
    sources = set()
    for B, C, hw, G, silu, acc_dx, acc_param, from_fwd, form in R.GN_BWD_CASES:
        forms = R.gn_bwd_forms(B, C, hw, G, silu, acc_dx, acc_param)
        assert form in forms, (B, C, hw, G, form, forms)
        seen |= forms
        sources.add(from_fwd)
    assert seen == R.GN_BWD_FORMS and sources == {False, True}
    assert R.gn_bwd_apply_cols_threads(320) == 240
    small = [c for c in R.GN_BWD_CASES if c[8].startswith("small")]
    assert {c[6] for c in small} == {0, 1}


def test_layernorm_backward_table_reaches_every_form():
    seen = set()
    for rows, d, ld, forms in R.LN_BWD_CASES:
        got = set()
        for scratch in (False, True):
            got |= R.ln_bwd_forms(rows, ld, scratch)[0]
        assert set(forms) <= got, (rows, ld, forms, got)
        seen |= got
    assert seen == R.LN_BWD_FORMS
    assert R.ln_bwd_forms(136, 384, True)[1:3] == (17, 3)
    assert R.ln_bwd_forms(2050, 96, True)[1] == 257
    assert R.ln_bwd_forms(12, 2048, False)[3] == 64 * 1024
    assert R.ln_bwd_scratch_floats(50, 384) == 0 and R.ln_bwd_scratch_floats(136, 384) == 17 * 2 * 384 + 32 * 2 * 384


def test_bounds_are_what_the_docstrings_say():
    ref = torch.tensor([0.0, 1.0, -2.0], dtype=torch.float64)
    assert torch.equal(R.fwd_bound(ref, 2.0), 2.0 ** -8 * ref.abs() + 2.0 ** -9)
    assert R.param_bound(128, 10.0) == (128 * 2.0 ** -24 + 2.0 ** -20) * 10.0
    assert R.slab_bound(1.0) == 3 * 2.0 ** -8
    assert R.worst_ratio(torch.tensor([0.0, 1.0]), torch.tensor([0.0, 2.0])) == 0.5
    assert math.isinf(R.worst_ratio(torch.tensor([1e-30]), torch.tensor([0.0])))
    rf = torch.tensor([2.0 ** -121, 2.0 ** -119, 0.5], dtype=torch.float64)
    assert ((0.0 - rf).abs() <= R.softmax_fwd_bound(rf)).tolist() == [True, False, False]      # under the floor `got` may be 0
