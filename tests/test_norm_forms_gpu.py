"""Every dispatch form of the norm and softmax entry points (csrc/norm_elem.hip, csrc/backward.hip) against the float64
references of tests/norm_ref.py, per element / per slab / per column, on benign and hostile inputs.  The tables, the inputs
and the bounds (with their derivations) live in norm_ref.py; test_norm_ref_cpu.py shows that the tables reach every form.
Every test prints its worst error / bound ratio."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import norm_ref as R  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402
from gpu_util import DEV, sync  # noqa: E402


def lib():
    return N.lib()


def dev_bf16(t):
    return t.to(torch.bfloat16).to(DEV)


def host(t):
    return t.float().cpu().double()


def report(entry, what, ratio):
    print("norm-forms %s %s worst error/bound = %.3f" % (entry, what, ratio))


def gn_id(c):
    return "B%d-C%d-hw%d-G%d" % tuple(c[:4])


def per_slab_max(t, G):
    B, hw, C = t.shape
    return t.abs().view(B, hw, G, C // G).amax(dim=(1, 3))


def check_stats(st, mean, rstd, entry, what):
    bm, br = R.stats_bounds(mean, rstd)
    st = st.cpu().double()
    rm = R.worst_ratio((st[..., 0] - mean).abs(), bm)
    rr = R.worst_ratio((st[..., 1] - rstd).abs(), br)
    report(entry, what + " mean", rm)
    report(entry, what + " rstd", rr)
    assert rm <= 1.0 and rr <= 1.0, (what, rm, rr)


# ------------------------------------------------------------------------------------------------ GroupNorm forward
@pytest.mark.parametrize("kind", R.GN_KINDS)
@pytest.mark.parametrize("case", R.GN_FWD_CASES, ids=gn_id)
def test_groupnorm_forward_every_form(case, kind):
    B, C, hw, G, _ = case
    L, s = lib(), N.stream_ptr()
    x = R.gn_input(kind, B, C, hw, G, "fwd.%d.%d.%d.%d" % (B, C, hw, G))
    gamma, beta = R.affine(C, "fwd")
    z_ref, mean, rstd = R.gn_forward_ref(x, G, gamma, beta, R.GN_EPS, False)
    refs = {0: z_ref, 1: R.silu64(z_ref)}
    if kind == "constant":
        flat = torch.tensor([[R.constant_slab(b, g) for g in range(G)] for b in range(B)])
        assert bool((rstd[flat] == 1.0 / math.sqrt(R.f32(R.GN_EPS))).all())       # variance exactly 0: rstd = 1 / sqrt(eps)
        bexp = beta.double().view(1, 1, G, C // G).expand(B, hw, G, C // G)[flat.view(B, 1, G, 1).expand(B, hw, G, C // G)]
        assert torch.equal(z_ref.view(B, hw, G, C // G)[flat.view(B, 1, G, 1).expand(B, hw, G, C // G)], bexp)   # y = beta
    xd, gd, bd = dev_bf16(x), gamma.to(DEV), beta.to(DEV)
    keep = xd.clone()
    scratch = torch.empty(L.ctta_groupnorm_scratch_floats(B, hw, C, G) + 16, device=DEV)
    em_mean, em_rstd = R.gn_stats_emulated(x, G)
    worst = 0.0
    for silu in (0, 1):
        ref = refs[silu]
        bound = R.fwd_bound(ref, R.slab_max(ref, G))
        outs = []
        for want_stats in (False, True):
            y = torch.full_like(xd, 9.0)
            st = torch.full((B, G, 2), float("nan"), device=DEV)
            if want_stats:
                N.check(L.ctta_groupnorm_stats_out(N.ptr(xd), N.ptr(y), B, hw, C, G, N.ptr(gd), N.ptr(bd), R.GN_EPS, silu,
                                                   N.ptr(scratch), N.ptr(st), s))
            else:
                N.check(L.ctta_groupnorm(N.ptr(xd), N.ptr(y), B, hw, C, G, N.ptr(gd), N.ptr(bd), R.GN_EPS, silu, N.ptr(scratch), s))
            sync()
            ratio = R.worst_ratio((host(y) - ref).abs(), bound)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (silu, want_stats, ratio)
            if want_stats:
                what = "%s %s silu=%d" % (gn_id(case), kind, silu)
                check_stats(st, mean, rstd, "groupnorm_stats_out", what)
                # the summation contract: fp32 running sums per channel and chunk, gn_group_fold's group fold, the chunks in fp64
                bm, br = R.emulation_bounds(mean, rstd)
                r_em = max(R.worst_ratio((st.cpu()[..., 0].double() - em_mean.double()).abs(), bm),
                           R.worst_ratio((st.cpu()[..., 1].double() - em_rstd.double()).abs(), br))
                report("groupnorm_stats_out", what + " vs the emulated order", r_em)
                assert r_em <= 1.0, (what, r_em)
            outs.append(y)
        assert torch.equal(outs[0], outs[1])             # asking for the statistics does not change the output
    assert torch.equal(xd, keep)
    report("groupnorm", "%s %s" % (gn_id(case), kind), worst)


@pytest.mark.parametrize("kind", ["benign", "offset64", "constant"])
@pytest.mark.parametrize("case", R.GN_PARTIALS_CASES, ids=lambda c: "B%d-C%d+%d-hw%d-G%d-stats%d" % tuple(c[:6]))
def test_groupnorm_from_partials_every_form(case, kind):
    B, C1, C2, hw, G, want_stats, _ = case
    C = C1 + C2
    L, s = lib(), N.stream_ptr()
    x = R.gn_input(kind, B, C, hw, G, "part.%d.%d.%d.%d" % (B, C, hw, G))
    gamma, beta = R.affine(C, "part")
    a, b = dev_bf16(x[..., :C1].contiguous()), dev_bf16(x[..., C1:].contiguous())
    gd, bd = gamma.to(DEV), beta.to(DEV)
    nchunk_expected = R.gn_geometry(hw, C)[1]
    cat = torch.empty(B, hw, C, dtype=torch.bfloat16, device=DEV)
    part = torch.full((B * nchunk_expected * G * 2,), float("nan"), device=DEV)
    nchunk = ctypes.c_int(0)
    N.check(L.ctta_concat_channels_gn(N.ptr(a), C1, N.ptr(b), C2, N.ptr(cat), B, hw, G, N.ptr(part), part.numel(),
                                      ctypes.byref(nchunk), s))
    sync()
    assert nchunk.value == nchunk_expected and torch.equal(cat, dev_bf16(x)) and bool(torch.isfinite(part).all())
    part_keep, cat_keep = part.clone(), cat.clone()
    scratch = torch.empty(L.ctta_groupnorm_scratch_floats(B, hw, C, G) + 16, device=DEV)
    scratch2 = torch.empty(B * 2 * C + 16, device=DEV)
    z_ref, mean, rstd = R.gn_forward_ref(x, G, gamma, beta, R.GN_EPS, False)
    worst = 0.0
    for silu in (0, 1):
        ref = R.silu64(z_ref) if silu else z_ref
        y_ref, y = torch.full_like(cat, 9.0), torch.full_like(cat, 9.0)
        st_ref, st = torch.zeros(B, G, 2, device=DEV), torch.zeros(B, G, 2, device=DEV)
        N.check(L.ctta_groupnorm_stats_out(N.ptr(cat), N.ptr(y_ref), B, hw, C, G, N.ptr(gd), N.ptr(bd), R.GN_EPS, silu,
                                           N.ptr(scratch), N.ptr(st_ref) if want_stats else None, s))
        N.check(L.ctta_groupnorm_from_partials(N.ptr(cat), N.ptr(y), B, hw, C, G, N.ptr(gd), N.ptr(bd), R.GN_EPS, silu,
                                               N.ptr(part), nchunk.value, N.ptr(scratch2), N.ptr(st) if want_stats else None, s))
        sync()
        assert torch.equal(y, y_ref) and torch.equal(st, st_ref)           # the same chunking and order: the same bits
        ratio = R.worst_ratio((host(y) - ref).abs(), R.fwd_bound(ref, R.slab_max(ref, G)))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (silu, ratio)
        if want_stats:
            check_stats(st, mean, rstd, "groupnorm_from_partials", "C%d+%d %s silu=%d" % (C1, C2, kind, silu))
    assert torch.equal(part, part_keep) and torch.equal(cat, cat_keep)
    report("groupnorm_from_partials", "C%d+%d-hw%d-stats%d %s" % (C1, C2, hw, want_stats, kind), worst)


# ------------------------------------------------------------------------------------------------ LayerNorm forward
@pytest.mark.parametrize("kind", R.GN_KINDS)
@pytest.mark.parametrize("case", R.LN_FWD_CASES, ids=lambda c: "rows%d-d%d-ld%d" % tuple(c[:3]))
def test_layernorm_forward_every_form(case, kind):
    rows, d, ld, _ = case
    x = R.rows_input(kind, rows, d, ld, "ln.%d.%d" % (rows, ld))
    gamma, beta = R.affine(d, "ln")
    ref = R.ln_forward_ref(x, d, gamma, beta, R.LN_EPS)
    if kind == "constant":
        assert torch.equal(ref[0::2, :d], beta.double().expand(len(range(0, rows, 2)), d))      # a constant row normalises to beta
    xd, gd, bd = dev_bf16(x), gamma.to(DEV), beta.to(DEV)
    keep = xd.clone()
    y = torch.full((rows, ld), 9.0, dtype=torch.bfloat16, device=DEV)
    N.check(lib().ctta_layernorm(N.ptr(xd), N.ptr(y), rows, d, ld, N.ptr(gd), N.ptr(bd), R.LN_EPS, N.stream_ptr()))
    sync()
    got = host(y)
    assert float(got[:, d:].abs().max()) == 0.0 if d < ld else True           # the pad columns are exactly zero
    M = ref.abs().amax(dim=1, keepdim=True)
    ratio = R.worst_ratio((got - ref).abs()[:, :d], R.fwd_bound(ref, M)[:, :d])
    report("layernorm", "rows%d-d%d-ld%d %s" % (rows, d, ld, kind), ratio)
    assert ratio <= 1.0
    assert torch.equal(xd, keep)


# ------------------------------------------------------------------------------------------------ softmax_rows
SOFTMAX_SCALE = 0.044


@pytest.mark.parametrize("kind", R.SOFTMAX_KINDS)
@pytest.mark.parametrize("case", R.SOFTMAX_CASES, ids=lambda c: "rows%d-cols%d" % tuple(c[:2]))
def test_softmax_rows_every_form(case, kind):
    rows, cols, _ = case
    sc = R.softmax_scores(kind, rows, cols, cols, SOFTMAX_SCALE, "sm.%d" % cols)
    ref = R.softmax_ref(sc, cols, SOFTMAX_SCALE)
    sd = sc.to(DEV)
    keep = sd.clone()
    p = torch.full((rows, cols), 9.0, dtype=torch.bfloat16, device=DEV)
    N.check(lib().ctta_softmax_rows(N.ptr(sd), N.ptr(p), rows, cols, SOFTMAX_SCALE, N.stream_ptr()))
    sync()
    got = p.float().cpu()
    ratio = R.worst_ratio((got.double() - ref).abs(), R.softmax_fwd_bound(ref))
    report("softmax_rows", "rows%d-cols%d %s" % (rows, cols, kind), ratio)
    assert ratio <= 1.0
    assert torch.equal(sd, keep)
    if kind == "equal":
        assert bool((got == got[:, :1]).all())          # equal scores: equal probabilities, whichever trip a column is in


@pytest.mark.parametrize("kind", R.SOFTMAX_KINDS)
def test_softmax_register_form_equals_the_generic_form_bit_for_bit(kind):
    """1024 columns run as 1024 (softmax_rows_reg_kernel<1>) and embedded in a 1028-column row (softmax_rows_kernel) whose four
    extra scores are -3e38: they take no part in the maximum and add + 0.0 to the sum, so the header's bit-identity shows."""
    rows, cols = 6, 1024
    sc = R.softmax_scores(kind, rows, cols, cols, SOFTMAX_SCALE, "sm.bits")
    wide = torch.full((rows, cols + 4), -3.0e38)
    wide[:, :cols] = sc
    L, s = lib(), N.stream_ptr()
    sd, wd = sc.to(DEV), wide.to(DEV)
    p, pw = (torch.full((rows, c), 9.0, dtype=torch.bfloat16, device=DEV) for c in (cols, cols + 4))
    N.check(L.ctta_softmax_rows(N.ptr(sd), N.ptr(p), rows, cols, SOFTMAX_SCALE, s))
    N.check(L.ctta_softmax_rows(N.ptr(wd), N.ptr(pw), rows, cols + 4, SOFTMAX_SCALE, s))
    sync()
    assert torch.equal(pw[:, :cols], p) and float(pw[:, cols:].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ GroupNorm backward
@pytest.mark.parametrize("kind", ["benign", "offset16", "constant"])
@pytest.mark.parametrize("case", R.GN_BWD_CASES, ids=lambda c: "%s-silu%d-accdx%d-accp%d-fwdstats%d" % ((gn_id(c),) + tuple(c[4:8])))
def test_groupnorm_backward_every_form(case, kind):
    B, C, hw, G, silu, acc_dx, acc_param, from_fwd, _ = case
    L, s = lib(), N.stream_ptr()
    tag = "bwd.%d.%d.%d.%d" % (B, C, hw, G)
    x = R.gn_input(kind, B, C, hw, G, tag)
    dy = R.bf16_round(R.det("nf.gn.dy." + tag, (B, hw, C), 4))
    gamma, beta = R.affine(C, "bwd")
    xd, dyd, gd, bd = dev_bf16(x), dev_bf16(dy), gamma.to(DEV), beta.to(DEV)
    stats = torch.full((B, G, 2), float("nan"), device=DEV)
    if from_fwd:
        ytmp = torch.empty_like(xd)
        fscratch = torch.empty(L.ctta_groupnorm_scratch_floats(B, hw, C, G) + 16, device=DEV)
        N.check(L.ctta_groupnorm_stats_out(N.ptr(xd), N.ptr(ytmp), B, hw, C, G, N.ptr(gd), N.ptr(bd), R.GN_EPS, silu,
                                           N.ptr(fscratch), N.ptr(stats), s))
    else:
        N.check(L.ctta_groupnorm_stats(N.ptr(xd), B, hw, C, G, R.GN_EPS, N.ptr(stats), s))
    sync()
    _, mean, rstd = R.gn_forward_ref(x, G, gamma, beta, R.GN_EPS, False)
    check_stats(stats, mean, rstd, "groupnorm_stats" if not from_fwd else "groupnorm_stats_out", "%s %s" % (gn_id(case), kind))
    # the reference works from the statistics the kernel is handed
    dx_ref, dg_ref, db_ref, ag, ab = R.gn_backward_ref(x, dy, G, gamma, beta, R.GN_EPS, silu, stats=stats.cpu())
    pre_dx = R.bf16_round(R.det("nf.gn.pre." + tag, (B, hw, C), 5) * 0.5)
    pre_g, pre_b = 0.5 + 0.25 * R.det("nf.gn.pg", (C,), 6), -0.25 + 0.5 * R.det("nf.gn.pb", (C,), 7)
    assert float(pre_g.abs().min()) > 0 and float(pre_b.abs().min()) > 0
    dx = dev_bf16(pre_dx) if acc_dx else torch.full_like(xd, 9.0)
    dg, dbt = pre_g.to(DEV), pre_b.to(DEV)               # accumulate_param = 0 must overwrite them
    keep = (xd.clone(), dyd.clone(), stats.clone())
    scratch = torch.empty(L.ctta_groupnorm_bwd_scratch_floats(B, hw, C, G), device=DEV)
    N.check(L.ctta_groupnorm_bwd(N.ptr(xd), N.ptr(dyd), N.ptr(dx), B, hw, C, G, N.ptr(stats), N.ptr(gd), N.ptr(bd), silu,
                                 acc_dx, N.ptr(dg), N.ptr(dbt), acc_param, N.ptr(scratch), s))
    sync()
    got = host(dx)
    assert bool(torch.isfinite(got).all())
    want = dx_ref + pre_dx.double() if acc_dx else dx_ref
    r_dx = R.worst_ratio(per_slab_max(got - want, G), R.slab_bound(per_slab_max(want, G)))
    n = B * hw
    want_g = dg_ref + pre_g.double() if acc_param else dg_ref
    want_b = db_ref + pre_b.double() if acc_param else db_ref
    r_g = R.worst_ratio((dg.cpu().double() - want_g).abs(), R.param_bound(n, ag))
    r_b = R.worst_ratio((dbt.cpu().double() - want_b).abs(), R.param_bound(n, ab))
    what = "%s silu=%d acc_dx=%d acc_param=%d %s" % (gn_id(case), silu, acc_dx, acc_param, kind)
    report("groupnorm_bwd", what + " dx", r_dx)
    report("groupnorm_bwd", what + " dgamma", r_g)
    report("groupnorm_bwd", what + " dbeta", r_b)
    assert r_dx <= 1.0 and r_g <= 1.0 and r_b <= 1.0, (r_dx, r_g, r_b)
    assert torch.equal(xd, keep[0]) and torch.equal(dyd, keep[1]) and torch.equal(stats, keep[2])


# ------------------------------------------------------------------------------------------------ LayerNorm backward
@pytest.mark.parametrize("kind", ["benign", "offset16", "constant"])
@pytest.mark.parametrize("case", R.LN_BWD_CASES, ids=lambda c: "rows%d-d%d-ld%d" % tuple(c[:3]))
def test_layernorm_backward_every_form(case, kind):
    rows, d, ld, _ = case
    L, s = lib(), N.stream_ptr()
    tag = "lnb.%d.%d" % (rows, ld)
    x = R.rows_input(kind, rows, d, ld, tag)
    dy = torch.full((rows, ld), 3.0)                     # pad columns of dy carry a value too: nothing may read them
    dy[:, :d] = R.det("nf.ln.dy." + tag, (rows, d), 4)
    dy = R.bf16_round(dy)
    gamma, _ = R.affine(d, "lnb")
    dx_ref, dg_ref, db_ref, ag, ab = R.ln_backward_ref(x, dy, d, gamma, R.LN_EPS)
    add = R.bf16_round(R.det("nf.ln.add." + tag, (rows, ld), 7))
    pre_g, pre_b = 0.5 + 0.25 * R.det("nf.ln.pg", (d,), 6), -0.25 + 0.5 * R.det("nf.ln.pb", (d,), 8)
    xd, dyd, gd, addd = dev_bf16(x), dev_bf16(dy), gamma.to(DEV), dev_bf16(add)
    keep = (xd.clone(), dyd.clone(), addd.clone())
    what = "rows%d-d%d-ld%d %s" % (rows, d, ld, kind)

    def params_ok(dg, dbt, name):
        r_g = R.worst_ratio((dg.cpu().double() - (dg_ref + pre_g.double())).abs(), R.param_bound(rows, ag))
        r_b = R.worst_ratio((dbt.cpu().double() - (db_ref + pre_b.double())).abs(), R.param_bound(rows, ab))
        report(name, what + " dgamma", r_g)
        report(name, what + " dbeta", r_b)
        assert r_g <= 1.0 and r_b <= 1.0, (name, r_g, r_b)

    def dx_ok(dx, want, name):
        got = host(dx)
        assert bool(torch.isfinite(got).all())
        r = R.worst_ratio((got - want).abs().amax(dim=1), R.slab_bound(want.abs().amax(dim=1)))
        report(name, what + " dx", r)
        assert r <= 1.0, (name, r)
        return got

    # plain: dgamma / dbeta hold a running sum and are added to (one block, or one atomic per block and column)
    dx0, dg0, db0 = torch.full_like(xd, 9.0), pre_g.to(DEV), pre_b.to(DEV)
    N.check(L.ctta_layernorm_bwd(N.ptr(xd), N.ptr(dyd), N.ptr(dx0), rows, d, ld, N.ptr(gd), R.LN_EPS, 0, N.ptr(dg0), N.ptr(db0), s))
    sync()
    got0 = dx_ok(dx0, dx_ref, "layernorm_bwd")
    assert float(got0[:, d:].abs().max()) == 0.0 if d < ld else True           # the pad columns are exactly zero
    params_ok(dg0, db0, "layernorm_bwd")
    # with a separate dx_add: untouched, and the in-place accumulate gives the same bits
    dx1, dg1, db1 = torch.full_like(xd, 9.0), pre_g.to(DEV), pre_b.to(DEV)
    N.check(L.ctta_layernorm_bwd_add(N.ptr(xd), N.ptr(dyd), N.ptr(addd), N.ptr(dx1), rows, d, ld, N.ptr(gd), R.LN_EPS, N.ptr(dg1),
                                     N.ptr(db1), s))
    inpl, dg2, db2 = addd.clone(), pre_g.to(DEV), pre_b.to(DEV)
    N.check(L.ctta_layernorm_bwd(N.ptr(xd), N.ptr(dyd), N.ptr(inpl), rows, d, ld, N.ptr(gd), R.LN_EPS, 1, N.ptr(dg2), N.ptr(db2), s))
    sync()
    assert torch.equal(addd, keep[2]) and torch.equal(dx1, inpl)
    want_add = dx_ref + add.double()                     # ln_backward_ref leaves the pads 0: there dx = dx_add
    dx_ok(dx1, want_add, "layernorm_bwd_add")
    assert torch.equal(dx1[:, d:], addd[:, d:])
    params_ok(dg1, db1, "layernorm_bwd_add")
    # with the caller's partial table where the shape has one: the same dx bit for bit, a fixed-order fold of dgamma / dbeta
    nf = int(L.ctta_layernorm_bwd_scratch_floats(rows, ld))
    assert nf == R.ln_bwd_scratch_floats(rows, ld)
    part = torch.full((max(nf, 1),), float("nan"), device=DEV)
    dx3, dg3, db3 = torch.full_like(xd, 9.0), pre_g.to(DEV), pre_b.to(DEV)
    N.check(L.ctta_layernorm_bwd_ws(N.ptr(xd), N.ptr(dyd), None, N.ptr(dx3), rows, d, ld, N.ptr(gd), R.LN_EPS, N.ptr(dg3), N.ptr(db3),
                                    N.ptr(part), nf, s))
    sync()
    assert torch.equal(dx3, dx0)
    params_ok(dg3, db3, "layernorm_bwd_ws")
    if nf:                                               # the fold is deterministic: a second run gives the same bits
        dx4, dg4, db4 = torch.full_like(xd, 9.0), pre_g.to(DEV), pre_b.to(DEV)
        N.check(L.ctta_layernorm_bwd_ws(N.ptr(xd), N.ptr(dyd), None, N.ptr(dx4), rows, d, ld, N.ptr(gd), R.LN_EPS, N.ptr(dg4),
                                        N.ptr(db4), N.ptr(part), nf, s))
        sync()
        assert torch.equal(dg4, dg3) and torch.equal(db4, db3) and torch.equal(dx4, dx0)
    assert torch.equal(xd, keep[0]) and torch.equal(dyd, keep[1])


# ------------------------------------------------------------------------------------------------ softmax with bias + backward
BIAS_SCALE = 0.14


@pytest.mark.parametrize("bias_kind", R.SOFTMAX_BIAS_KINDS)
@pytest.mark.parametrize("case", R.SOFTMAX_BIAS_CASES, ids=lambda c: "rows%d-cols%d-ldp%d-rpb%d-lds%d-bias%d" % tuple(c))
def test_softmax_bias_forward_and_backward(case, bias_kind):
    rows, cols, ldp, rpb, lds, with_bias = case
    L, s = lib(), N.stream_ptr()
    sc = R.softmax_scores("benign", rows, cols, lds, BIAS_SCALE, "sb.%d.%d" % (cols, lds))
    sc[:, :cols] *= 8.0 / 30.0                           # +- 8, today's
    bias = R.softmax_bias(bias_kind, rows // rpb, cols) if with_bias else None
    ref = R.softmax_ref(sc, cols, BIAS_SCALE, bias, rpb)
    sd = sc.to(DEV)
    bd = bias.to(DEV) if with_bias else None
    pd = torch.full((rows, ldp), 9.0, dtype=torch.bfloat16, device=DEV)
    keep_s = sd.clone()
    N.check(L.ctta_softmax_bias_rows(N.ptr(sd), lds, N.ptr(bd), rpb, N.ptr(pd), rows, cols, ldp, BIAS_SCALE, s))
    sync()
    got = pd.float().cpu()
    assert float(got[:, cols:].abs().max()) == 0.0       # the pad columns are exactly zero
    r_p = R.worst_ratio((got[:, :cols].double() - ref).abs(), R.softmax_fwd_bound(ref))
    what = "rows%d-cols%d-lds%d-bias%d %s" % (rows, cols, lds, with_bias, bias_kind)
    report("softmax_bias_rows", what, r_p)
    assert r_p <= 1.0
    assert torch.equal(sd, keep_s)
    # backward from the bf16 P the kernel is given
    dp = torch.full((rows, lds), 1.0e30)
    dp[:, :cols] = R.det("nf.sb.dp.%d" % cols, (rows, cols), 2)
    dpd = dp.to(DEV)
    ds = torch.full((rows, ldp), 9.0, dtype=torch.bfloat16, device=DEV)
    keep_p, keep_dp = pd.clone(), dpd.clone()
    N.check(L.ctta_softmax_bwd_rows(N.ptr(pd), N.ptr(dpd), lds, N.ptr(ds), rows, cols, ldp, BIAS_SCALE, s))
    sync()
    ds_ref, dot_abs = R.softmax_backward_ref(got, dp, cols, BIAS_SCALE)
    gds = host(ds)
    assert float(gds[:, cols:].abs().max()) == 0.0
    err = (gds[:, :cols] - ds_ref).abs()
    r_el = R.worst_ratio(err, R.softmax_bwd_bound(ds_ref, got[:, :cols], dot_abs, cols, BIAS_SCALE))
    r_row = R.worst_ratio(err.amax(dim=1), R.slab_bound(ds_ref.abs().amax(dim=1)))
    report("softmax_bwd_rows", what + " per element", r_el)
    report("softmax_bwd_rows", what + " per row", r_row)
    assert r_el <= 1.0 and r_row <= 1.0, (r_el, r_row)
    assert torch.equal(pd, keep_p) and torch.equal(dpd, keep_dp)
