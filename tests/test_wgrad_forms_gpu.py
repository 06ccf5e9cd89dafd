"""Every route of the weight-gradient kernels (csrc/wgrad_gemm.hip, ctta_im2col_t + conv_gemm, ctta_wgrad_rowsum, the scatter
step of csrc/backward.hip) against the float64 references of tests/wgrad_ref.py, PER ELEMENT: |got - ref| <= 2^-24 (L A + |ref|)
on zero-mean and on all-positive inputs, exact equality on impulses, the column sums bit for bit against the emulated
summation order, NaN in everything a kernel may address but must not use.  The table, the inputs, the bounds (with their
derivation) and the launch mirror live in wgrad_ref.py; test_wgrad_ref_cpu.py shows that the table reaches every class.
Every test prints its worst |diff| / bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import wgrad_ref as R  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402
from gpu_util import DEV, sync  # noqa: E402

NAN = float("nan")


def lib():
    return N.lib()


def params(kind):
    ps = [(c, f) for c, f in R.case_params() if c["kind"] == kind]
    return dict(argnames="c,family", argvalues=ps, ids=["%s-%s" % (c["id"], f) for c, f in ps])


def report(form, family, what, ratio):
    print("wgrad-forms %s %s %s worst |diff|/bound = %.3f" % (form, family, what, ratio))


def inside(form, family, what, got, ref, A, L):
    ratio = R.worst_ratio((got.double().cpu() - ref).abs(), R.bound(L, A, ref))
    report(form, family, what, ratio)
    assert ratio <= 1.0, (form, what, ratio)


def check_slabs(form, family, slabs, r, K, M, S, seg, nb, bias, sums=None, sums_L=0, gemm_splits=0, gemm_cols=0):
    """One launch's slabs (S, N, ld) against the per-split references `r`: poison, per-slab and folded bounds (or equality),
    empty splits, and the column sums against their emulation `sums` = (bias (S, N), ps (S, B, N) or None).
    `gemm_cols`: conv_gemm stores whole groups of four channels (include/ctta.h: n need not be a multiple of 4 when
    round_up(n, 4) <= ldc), so where the GEMM itself writes the bias and per-sample columns its store owns the slab up to
    round_up(rows, 4): those pad columns must then hold exactly 0.0 (zero weight rows), everything behind them its fill."""
    sl = slabs.cpu()
    used = K + (1 + nb if bias else 0)
    owned = max(used, gemm_cols)
    assert bool((sl[:, :, used:owned] == 0.0).all()), "%s: the GEMM's pad columns must be exactly 0" % form
    assert bool(torch.isnan(sl[:, :, owned:]).all()), "%s wrote behind its columns" % form
    assert bool(torch.isfinite(sl[:, :, :used]).all()), "%s: a poisoned or unwritten value reached a used column" % form
    dw = sl[:, :, :K].double()
    for s in range(S):
        if s * seg >= M:
            assert bool((sl[s, :, :used] == 0.0).all()), "%s: split %d holds no position and must be exactly 0" % (form, s)
    if family == "impulse":
        assert torch.equal(dw, r["dw"]) and torch.equal(dw.sum(0), r["dw"].sum(0)), form
    else:
        inside(form, family, "dW per slab", dw, r["dw"], r["adw"], R.L_mfma(seg, 1, conv_splits=gemm_splits))
        inside(form, family, "dW folded", dw.sum(0), r["dw"].sum(0), r["adw"].sum(0), R.L_mfma(seg, S, conv_splits=gemm_splits))
    if not bias:
        return
    db = sl[:, :, K]
    ps = sl[:, :, K + 1:K + 1 + nb].permute(0, 2, 1)
    if sums is not None:
        assert torch.equal(db, sums[0]), "%s: bias column differs from the emulated summation order" % form
        if nb:
            assert torch.equal(ps, sums[1][:, :nb]), "%s: per-sample columns differ from the emulated summation order" % form
    inside(form, family, "db per slab", db, r["db"], r["adb"], sums_L)
    inside(form, family, "db folded", db.double().sum(0), r["db"].sum(0), r["adb"].sum(0), sums_L)
    if nb:
        inside(form, family, "ps per slab", ps, r["ps"][:, :nb], r["aps"][:, :nb], sums_L)
        inside(form, family, "ps folded", ps.double().sum(0), r["ps"][:, :nb].sum(0), r["aps"][:, :nb].sum(0), sums_L)


def scatter_one_slab(L, st, slab, ld, K, Nn, pm, bias, co=None):
    """slab (1, N, ld) -> zero gradients through ctta_wgrad_scatter_rows_bias(accumulate = 1)."""
    gw, gb = torch.zeros(Nn * pm["kd"], device=DEV), torch.zeros(Nn, device=DEV)
    N.check(L.ctta_wgrad_scatter_rows_bias(N.ptr(slab), 1, Nn * ld, ld, K, Nn, N.ptr(pm["ro_d"]), N.ptr(co), N.ptr(gw),
                                           K if bias else -1, Nn if bias else 0, N.ptr(pm["bidx_d"]) if bias else None,
                                           N.ptr(gb) if bias else None, 1, st))
    return gw, gb


def on_device(pm):
    """The maps of a pack map on the device, kept alive by the dict for as long as launches read them."""
    pm["ro_d"], pm["bidx_d"] = pm["ro"].to(DEV), pm["bidx"].to(DEV)
    pm["co_d"] = pm["co"].to(DEV) if pm["co"] is not None else None
    return pm


# ------------------------------------------------------------------------------------------------ implicit 3x3: three forms
@pytest.mark.parametrize(**params("i3"))
def test_implicit_3x3_every_form(c, family):
    L, st = lib(), N.stream_ptr()
    p = R.forced_plan(c)
    S, mp, seg, ld = p["splits"], p["mp"], p["seg"], p["ld"]
    B, C, H, W, Nn, nb, bias = c["B"], c["C"], c["H"], c["W"], c["N"], c["nb"], c["bias"]
    M, K, HW = B * H * W, 9 * C, H * W
    kern = R.implicit_kernel(9, W, True).split("<")[0]
    x, dy = R.make_inputs(c, family, S, seg)
    r = R.split_refs(x, dy, c, S, seg)
    xd, dyd = R.dev_matrix(x.view(M, C), c["x_ld"], DEV), R.dev_matrix(dy, c["ldy"], DEV)
    keep_x, keep_dy = xd.clone(), dyd.clone()
    bias_col = K if bias else -1
    # dY^T form (+ ctta_wgrad_rowsum's kernel for the column sums)
    pt = torch.full((Nn, mp), NAN, dtype=torch.bfloat16, device=DEV)
    N.check(L.ctta_transpose_bf16(N.ptr(dyd), 0, M, Nn, c["ldy"], 0, N.ptr(pt), 0, mp, 1, st))
    slabs_t = torch.full((S, Nn, ld), NAN, device=DEV)
    N.check(L.ctta_wgrad_implicit(N.ptr(pt), Nn, mp, N.ptr(xd), c["x_ld"], C, B, H, W, 9, M, S, bias_col, nb, N.ptr(slabs_t), Nn * ld,
                                  ld, st))
    # dY in place
    slabs_n = torch.full((S, Nn, ld), NAN, device=DEV)
    N.check(L.ctta_wgrad_implicit_inplace(N.ptr(dyd), c["ldy"], Nn, mp, N.ptr(xd), c["x_ld"], C, B, H, W, 9, M, S, bias_col, nb,
                                          N.ptr(slabs_n), Nn * ld, ld, st))
    sync()
    assert torch.equal(pt[:, :M].cpu(), dy.t().to(torch.bfloat16)) and bool((pt[:, M:] == 0).all())
    check_slabs(kern + "<dyt>", family, slabs_t, r, K, M, S, seg, nb, bias, R.emu_sums_rowsum(dy, M, mp, S, HW, nb, B),
                R.sums_L_rowsum(seg, S, nb))
    check_slabs(kern + "<nat>", family, slabs_n, r, K, M, S, seg, nb, bias, R.emu_sums_implicit(dy, M, mp, S, HW, nb, B),
                R.sums_L_implicit(seg, S, HW, nb))
    assert torch.equal(slabs_n[:, :, :K], slabs_t[:, :, :K]), "dY in place and dY^T: the same MFMA products in the same order"
    # direct: one split, no per-sample columns, against slab + scatter of the same launch shape
    mp1, ld1 = R.rup(M, 64), R.rup(K + 1, 4)
    slab1 = torch.full((1, Nn, ld1), NAN, device=DEV)
    N.check(L.ctta_wgrad_implicit_inplace(N.ptr(dyd), c["ldy"], Nn, mp1, N.ptr(xd), c["x_ld"], C, B, H, W, 9, M, 1, bias_col, 0,
                                          N.ptr(slab1), Nn * ld1, ld1, st))
    pm = on_device(R.pack_map(c, drop_row=1))
    gw_s, gb_s = scatter_one_slab(L, st, slab1, ld1, K, Nn, pm, bias)
    gw_d, gb_d = torch.zeros(Nn * K, device=DEV), torch.zeros(Nn, device=DEV)
    N.check(L.ctta_wgrad_implicit_direct(N.ptr(dyd), c["ldy"], Nn, mp1, N.ptr(xd), c["x_ld"], C, B, H, W, M, K, Nn,
                                         N.ptr(pm["ro_d"]), N.ptr(gw_d), Nn, N.ptr(pm["bidx_d"]),
                                         N.ptr(gb_d) if bias else None, st))
    sync()
    assert torch.equal(gw_d, gw_s) and torch.equal(gb_d, gb_s), "direct = slab + scatter(accumulate = 1), bit for bit"
    r1 = R.split_refs(x, dy, c, 1, mp1)
    keep = torch.ones(Nn, dtype=torch.bool)
    keep[1] = False
    got = gw_d.view(Nn, K).cpu()
    assert bool((got[~keep] == 0).all()) and float(gb_d[1]) == 0.0          # the padding row and its bias slot: untouched
    if family == "impulse":
        assert torch.equal(got[keep].double(), r1["dw"][0][keep])
    else:
        inside(kern + "<direct>", family, "dW", got[keep], r1["dw"][0][keep], r1["adw"][0][keep], R.L_mfma(mp1, 1, direct=True))
    if bias:
        em = R.emu_sums_implicit(dy, M, mp1, 1, HW, 0, B)[0][0]
        assert torch.equal(gb_d.cpu()[keep], em[keep])
        inside(kern + "<direct>", family, "db", gb_d.cpu()[keep], r1["db"][0][keep], r1["adb"][0][keep], R.sums_L_implicit(mp1, 1, HW, 0) + 1)
    else:
        assert float(gb_d.abs().max()) == 0.0
    # the operands are read only; their poison is where it was
    for t, k in ((xd, keep_x), (dyd, keep_dy)):
        assert torch.equal(t.view(torch.int16), k.view(torch.int16))


# ------------------------------------------------------------------------------------------------ both operands in place
@pytest.mark.parametrize(**params("tn"))
def test_linear_in_place_every_form(c, family):
    L, st = lib(), N.stream_ptr()
    p = R.forced_plan(c)
    S, mp, seg = p["splits"], p["mp"], p["seg"]
    C, Nn, bias = c["C"], c["N"], c["bias"]
    M, K = c["H"], C
    ld = R.rup(K + 1, 4)
    x, dy = R.make_inputs(c, family)
    r = R.split_refs(x, dy, c, S, seg)
    xd, dyd = R.dev_matrix(x.view(M, C), c["x_ld"], DEV), R.dev_matrix(dy, c["ldy"], DEV)
    slabs = torch.full((S, Nn, ld), NAN, device=DEV)
    N.check(L.ctta_wgrad_tn(N.ptr(dyd), c["ldy"], Nn, N.ptr(xd), c["x_ld"], C, M, mp, S, K if bias else -1, N.ptr(slabs), Nn * ld, ld, st))
    sync()
    check_slabs("tn", family, slabs, r, K, M, S, seg, 0, bias, (R.emu_sums_tn(dy, M, mp, S), None), R.sums_L_tn(seg, S))
    # direct, with the identity map and with a column map that drops the first and the last column
    mp1 = R.rup(M, 64)
    r1 = R.split_refs(x, dy, c, 1, mp1)
    slab1 = torch.full((1, Nn, ld), NAN, device=DEV)
    N.check(L.ctta_wgrad_tn(N.ptr(dyd), c["ldy"], Nn, N.ptr(xd), c["x_ld"], C, M, mp1, 1, K if bias else -1, N.ptr(slab1), Nn * ld, ld, st))
    for colmap in (False, True):
        pm = on_device(R.pack_map(dict(c, colmap=colmap), drop_row=0))
        co = pm["co_d"]
        gw_s, gb_s = scatter_one_slab(L, st, slab1, ld, K, Nn, pm, bias, co)
        gw_d, gb_d = torch.zeros(Nn * pm["kd"], device=DEV), torch.zeros(Nn, device=DEV)
        N.check(L.ctta_wgrad_tn_direct(N.ptr(dyd), c["ldy"], Nn, N.ptr(xd), c["x_ld"], C, M, mp1, K, Nn, N.ptr(pm["ro_d"]), N.ptr(co),
                                       N.ptr(gw_d), Nn, N.ptr(pm["bidx_d"]), N.ptr(gb_d) if bias else None, st))
        sync()
        assert torch.equal(gw_d, gw_s) and torch.equal(gb_d, gb_s), colmap
        got = gw_d.view(Nn, pm["kd"]).cpu()
        cols = slice(1, K - 1) if colmap else slice(0, K)
        assert bool((got[0] == 0).all()) and float(gb_d[0]) == 0.0
        if Nn > 1:
            inside("tn<direct>", family, "dW", got[1:], r1["dw"][0][1:, cols], r1["adw"][0][1:, cols], R.L_mfma(mp1, 1, direct=True))
            if bias:
                assert torch.equal(gb_d.cpu()[1:], R.emu_sums_tn(dy, M, mp1, 1)[0][1:])
                inside("tn<direct>", family, "db", gb_d.cpu()[1:], r1["db"][0][1:], r1["adb"][0][1:], R.sums_L_tn(mp1, 1) + 1)
        if not bias:
            assert float(gb_d.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ implicit kernel, one tap
@pytest.mark.parametrize(**params("i1"))
def test_implicit_one_tap(c, family):
    L, st = lib(), N.stream_ptr()
    p = R.forced_plan(c)
    S, mp, seg, ld = p["splits"], p["mp"], p["seg"], p["ld"]
    C, Nn, bias = c["C"], c["N"], c["bias"]
    M, K = c["H"], C
    x, dy = R.make_inputs(c, family)
    r = R.split_refs(x, dy, c, S, seg)
    xd, dyd = R.dev_matrix(x.view(M, C), c["x_ld"], DEV), R.dev_matrix(dy, c["ldy"], DEV)
    pt = torch.full((Nn, mp), NAN, dtype=torch.bfloat16, device=DEV)
    N.check(L.ctta_transpose_bf16(N.ptr(dyd), 0, M, Nn, c["ldy"], 0, N.ptr(pt), 0, mp, 1, st))
    slabs = torch.full((S, Nn, ld), NAN, device=DEV)
    N.check(L.ctta_wgrad_implicit(N.ptr(pt), Nn, mp, N.ptr(xd), c["x_ld"], C, 1, M, 1, 1, M, S, K if bias else -1, 0, N.ptr(slabs), Nn * ld,
                                  ld, st))
    sync()
    check_slabs("generic<1>", family, slabs, r, K, M, S, seg, 0, bias, R.emu_sums_rowsum(dy, M, mp, S, M, 0, 1), R.sums_L_rowsum(seg, S, 0))


# ------------------------------------------------------------------------------------------------ row sums alone
@pytest.mark.parametrize(**params("rowsum"))
def test_rowsum(c, family):
    L, st = lib(), N.stream_ptr()
    p = R.forced_plan(c)
    S, mp, seg, ld = p["splits"], p["mp"], p["seg"], p["ld"]
    B, Nn, nb, K = c["B"], c["N"], c["nb"], c["C"]
    M = R.positions(c)
    hw = M // B
    _, dy = R.make_inputs(c, family)
    r = R.split_refs(torch.zeros(B, c["H"], 1, K), dy, c, S, seg)
    dyt = torch.full((Nn, mp), NAN, dtype=torch.bfloat16, device=DEV)          # the pad behind M is never read
    dyt[:, :M] = dy.t().to(torch.bfloat16).to(DEV)
    slabs = torch.full((S, Nn, ld), NAN, device=DEV)
    N.check(L.ctta_wgrad_rowsum(N.ptr(dyt), Nn, mp, M, S, hw, nb, N.ptr(slabs), Nn * ld, ld, K, st))
    sync()
    sl = slabs.cpu()
    assert bool(torch.isnan(sl[:, :, :K]).all()) and bool(torch.isnan(sl[:, :, K + 1 + nb:]).all())
    em_b, em_p = R.emu_sums_rowsum(dy, M, mp, S, hw, nb, B)
    db, ps = sl[:, :, K], sl[:, :, K + 1:K + 1 + nb].permute(0, 2, 1)
    assert torch.equal(db, em_b) and torch.equal(ps, em_p[:, :nb])
    Ls = R.sums_L_rowsum(seg, S, nb)
    inside("rowsum", family, "db per slab", db, r["db"], r["adb"], Ls)
    inside("rowsum", family, "db folded", db.double().sum(0), r["db"].sum(0), r["adb"].sum(0), Ls)
    if nb:
        inside("rowsum", family, "ps per slab", ps, r["ps"][:, :nb], r["aps"][:, :nb], Ls)


# ------------------------------------------------------------------------------------------------ a layer as the engine runs it
@pytest.mark.parametrize(**params("mirror"))
def test_layer_through_plan_launch_and_scatter(c, family):
    L = lib()
    B, C, Nn, nb = c["B"], c["C"], c["N"], c["nb"]
    M, K = R.positions(c), c["kh"] * c["kw"] * c["C"]
    hw = M // B
    x, dy = R.make_inputs(c, family)
    xd, dyd = R.dev_matrix(x.view(-1, C), C, DEV), R.dev_matrix(dy, Nn, DEV)
    pm = R.pack_map(c)
    res = R.run_layer(L, c, R.POLICIES[c["policy"]], xd, dyd, pm, DEV)
    pl = res["plan"]
    route, S, seg, mp = R.ROUTES[pl.route], pl.splits, pl.seg, pl.mp
    assert dict(route=route, splits=S, mp=mp, seg=seg, rows=pl.rows, ld=pl.ld, sums_apart=pl.sums_apart,
                upsample_copy=pl.upsample_copy) == R.plan_py(R.geom_fields(c), R.POLICIES[c["policy"]])
    r = R.split_refs(x, dy, c, S, seg)
    direct = route.endswith("direct")
    gs = R.gemm_splits(L, Nn, K if pl.sums_apart else pl.rows, S, seg, mp, pl.ld) if route == "im2col_t" else 0
    form = "plan:" + route
    sums, Ls = None, R.L_mfma(seg, S, conv_splits=gs)          # indicator rows of the GEMM: a product like the others
    if route.startswith("implicit") and route != "implicit_dyt":
        sums, Ls = R.emu_sums_implicit(dy, M, mp, S, hw, nb, B), R.sums_L_implicit(seg, S, hw, nb)
    elif route.startswith("tn"):
        sums, Ls = (R.emu_sums_tn(dy, M, mp, S), None), R.sums_L_tn(seg, S)
    elif route == "implicit_dyt" or pl.sums_apart:
        sums, Ls = R.emu_sums_rowsum(dy, M, mp, S, hw, nb, B), R.sums_L_rowsum(seg, S, nb)
    if route == "im2col_t":          # the operand the GEMM reads: im2col^T bit for bit, zero pad, then the indicator rows
        q = res["q"].view(pl.rows, mp).cpu()
        assert torch.equal(q[:K, :M], R.unfold64(x, c).t().to(torch.bfloat16)) and bool((q[:K + 1 + nb, M:] == 0).all())
        assert bool((q[K, :M] == 1).all())
        for b in range(nb):
            want = (torch.arange(M) // hw == b).to(torch.bfloat16)
            assert torch.equal(q[K + 1 + b, :M], want)
    if res["slabs"] is not None:
        check_slabs(form, family, res["slabs"], r, K, M, S, seg, nb, True, sums, Ls, gs,
                    R.rup(pl.rows, 4) if route == "im2col_t" and not pl.sums_apart else 0)
    # the gradients the scatter leaves (zero before): the slabs folded in slab order, the bias through a wave butterfly
    cols = slice(1, K - 1) if c.get("colmap") else slice(0, K)
    inside(form, family, "grad_w", res["gw"], r["dw"].sum(0)[:, cols], r["adw"].sum(0)[:, cols], R.L_mfma(seg, S, direct, gs))
    inside(form, family, "grad_b", res["gb"], r["db"].sum(0), r["adb"].sum(0), Ls + 7)
    if nb:
        inside(form, family, "per-sample", res["ps"], r["ps"][:, :nb].sum(0), r["aps"][:, :nb].sum(0), Ls)
    if direct and sums is not None:
        assert torch.equal(res["gb"].cpu(), sums[0][0])
