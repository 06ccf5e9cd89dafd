"""tests/wgrad_ref.py checked on the CPU: the float64 references against torch.autograd, the absolute sums against the
references, fp32 emulations of the product and of the three column-sum orders against the bounds (the reference arithmetic
alone must stay well inside them, or a kernel could not), and the case table against the dispatch predicates and the real
ctta_wgrad_plan: every class the table promises, every plan route under every policy that reaches it, and the geometry
classes of the real layers of tests/golden/wgrad_plan_cases.json."""
import json
import os

import pytest
import torch

import wgrad_ref as R
from consistencytta_amd import _native as N
from test_wgrad_plan_cpu import REACHES, ROUTES as PLAN_ROUTES

assert tuple(PLAN_ROUTES) == tuple(R.ROUTES)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMERIC = [(c, f) for c, f in R.case_params() if f != "impulse"]
IDS = ["%s-%s" % (c["id"], f) for c, f in NUMERIC]
PRODUCTS = [(c, f) for c, f in NUMERIC if c["kind"] != "rowsum"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def plan_of(lib, c):
    """splits / mp / seg of a case: forced, or what the real plan says."""
    if c["kind"] != "mirror":
        return R.forced_plan(c)
    pl = R.plan_real(lib, R.geom_fields(c), R.POLICIES[c["policy"]])
    return dict(route=R.ROUTES[pl.route], splits=pl.splits, mp=pl.mp, seg=pl.seg, rows=pl.rows, ld=pl.ld,
                sums_apart=pl.sums_apart, upsample_copy=pl.upsample_copy)


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("c,family", PRODUCTS, ids=["%s-%s" % (c["id"], f) for c, f in PRODUCTS])
def test_split_references_sum_to_autograd_in_float64(lib, c, family):
    p = plan_of(lib, c)
    x, dy = R.make_inputs(c, family)
    r = R.split_refs(x, dy, c, p["splits"], p["seg"])
    dw, db, ps, adw, adb, aps = R.autograd_refs(x, dy, c)
    for got, ref in ((r["dw"], dw), (r["db"], db), (r["ps"], ps), (r["adw"], adw), (r["adb"], adb), (r["aps"], aps)):
        assert float((got.sum(0) - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    for k in ("dw", "db", "ps"):
        assert bool((r["a" + k] >= r[k].abs()).all())
        assert bool((r["a" + k].sum(0) >= r[k].sum(0).abs()).all())
    if family == "offset":          # every term is positive: A = ref, the test is a count of terms
        assert torch.equal(r["adw"], r["dw"]) and torch.equal(r["adb"], r["db"])


def test_impulse_gradient_is_one_dy_value_or_zero(lib):
    for cid in ("i3-W2-HW64", "i3-W8-S4", "i3-W64-S3"):
        c = R.BY_ID[cid]
        p = R.forced_plan(c)
        x, dy = R.make_inputs(c, "impulse", p["splits"], p["seg"])
        sites = R.impulse_sites(c, p["splits"], p["seg"])
        assert int(x.sum()) == len(sites) == int((x != 0).sum())
        assert len({R.impulse_channel(i, c["C"]) for i in range(len(sites))}) == len(sites) and R.impulse_channel(len(sites) - 1, c["C"]) >= 0
        dw = R.split_refs(x, dy, c, p["splits"], p["seg"])["dw"].sum(0).view(c["N"], c["C"], 9)
        vals = set(dy.view(-1).tolist()) | {0.0}
        assert set(dw.view(-1).tolist()) <= vals
        # the first site is the corner (0, 0, 0): taps that would reach outside the image see nothing
        ch = R.impulse_channel(0, c["C"])
        for t in range(9):
            oh, ow = 1 - t // 3, 1 - t % 3                      # the output pixel whose tap t lands on (0, 0)
            inside = 0 <= oh < c["H"] and 0 <= ow < c["W"]
            want = dy[oh * c["W"] + ow].double() if inside else torch.zeros(c["N"], dtype=torch.float64)
            assert torch.equal(dw[:, ch, t], want), (cid, t)


# ------------------------------------------------------------------------------------------------ emulations vs bounds
@pytest.mark.parametrize("c,family", PRODUCTS, ids=["%s-%s" % (c["id"], f) for c, f in PRODUCTS])
def test_fp32_emulation_of_the_product_stays_inside_half_of_the_bound(lib, c, family):
    p = plan_of(lib, c)
    S, seg = p["splits"], p["seg"]
    x, dy = R.make_inputs(c, family)
    r = R.split_refs(x, dy, c, S, seg)
    for k in ("dw", "db", "ps"):          # A >= |ref|, per split and folded, on every case of the table
        assert bool((r["a" + k] >= r[k].abs()).all()) and bool((r["a" + k].sum(0) >= r[k].sum(0).abs()).all())
    em = R.emu_products(x, dy, c, S, seg)
    ratio = R.worst_ratio((em - r["dw"].sum(0)).abs(), R.bound(R.L_mfma(seg, S), r["adw"].sum(0), r["dw"].sum(0)))
    print("wgrad-ref %s %s emulated product error/bound = %.3f" % (c["id"], family, ratio))
    assert ratio <= 0.5


@pytest.mark.parametrize("c,family", NUMERIC, ids=IDS)
def test_emulated_column_sums_stay_inside_their_bounds(lib, c, family):
    p = plan_of(lib, c)
    S, seg, mp = p["splits"], p["seg"], p["mp"]
    M, B = R.positions(c), c["B"]
    hw = M // B
    x, dy = R.make_inputs(c, family)
    r = R.split_refs(x, dy, c, S, seg)
    assert bool((r["adb"] >= r["db"].abs()).all()) and bool((r["aps"] >= r["ps"].abs()).all())
    forms = []
    if c["kind"] in ("i3", "mirror") and c["kh"] == 3 and hw % 64 == 0 and mp % (64 * S) == 0:
        forms.append(("implicit", R.emu_sums_implicit(dy, M, mp, S, hw, c["nb"], B), R.sums_L_implicit(seg, S, hw, c["nb"])))
    if c["kind"] in ("tn", "mirror") and c["kh"] == 1:
        forms.append(("tn", (R.emu_sums_tn(dy, M, mp, S), None), R.sums_L_tn(seg, S)))
    if c["nb"] == 0 or hw % 8 == 0:
        forms.append(("rowsum", R.emu_sums_rowsum(dy, M, mp, S, hw, c["nb"], B), R.sums_L_rowsum(seg, S, c["nb"])))
    assert forms or (c["nb"] > 0 and hw % 8 != 0)          # only there do the sums ride in the GEMM as indicator rows
    for name, (bias, ps), L in forms:
        rb = R.worst_ratio((bias.double().sum(0) - r["db"].sum(0)).abs(), R.bound(L, r["adb"].sum(0), r["db"].sum(0)))
        rs = R.worst_ratio((bias.double() - r["db"]).abs(), R.bound(L, r["adb"], r["db"]))
        assert rb <= 1.0 and rs <= 1.0, (name, rb, rs)
        if ps is not None and c["nb"] > 0:
            nb = c["nb"]
            rp = R.worst_ratio((ps.double()[:, :nb] - r["ps"][:, :nb]).abs(), R.bound(L, r["aps"][:, :nb], r["ps"][:, :nb]))
            assert rp <= 1.0, (name, rp)
            assert float(ps[:, nb:].abs().max()) == 0.0 if nb < B else True
        print("wgrad-ref %s %s %s sums error/bound = %.3f (per slab %.3f)" % (c["id"], family, name, rb, rs))


def test_a_block_of_eight_rounds_on_spread_inputs_and_not_on_uniform_ones():
    """Why the row-sum cases also run `spread`: the tree sum of eight positions is exact on the zero-mean draw."""
    c = R.BY_ID["rs-M512-B2-nb0-S1"]
    for family, exact in (("uniform", True), ("spread", False)):
        d = R.make_inputs(c, family)[1].numpy().reshape(-1, 8, c["N"])
        f = [d[:, i] for i in range(8)]
        tree = ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]))
        other = ((f[0] + f[2]) + (f[1] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]))
        assert bool((tree == other).all()) == exact, family


def test_the_three_summation_orders_differ_where_they_should():
    """The emulations are three different orders, not one: on a long zero-mean column their fp32 results differ pairwise.
    (The `offset` column sums are exact in fp32 in any order -- multiples of 2^-6 below 2^18 -- they count terms instead.)"""
    c = R.BY_ID["tn-M1088-S8"]
    _, dy = R.make_inputs(c, "uniform")
    a = R.emu_sums_tn(dy, 1088, 1536, 1)
    b, _ = R.emu_sums_implicit(dy, 1088, 1536, 1, 1088, 0, 1)
    d, _ = R.emu_sums_rowsum(dy, 1088, 1536, 1, 1088, 0, 1)
    assert not torch.equal(a, b) and not torch.equal(b, d) and not torch.equal(a, d)


# ------------------------------------------------------------------------------------------------ the table
def test_predicates_agree_with_the_library(lib):
    for taps in (1, 9, 4):
        for c in (8, 24, 32, 36, 40, 264):
            for h, w in ((1, 64), (2, 64), (8, 8), (6, 4), (16, 4), (32, 2), (2, 32), (4, 16), (8, 48), (1, 128), (64, 1), (77, 1)):
                for x_ld in (c, c + 4, c + 8):
                    for n in (4, 8, 24):
                        assert bool(lib.ctta_wgrad_implicit_supported(taps, c, h, w, x_ld, n)) == R.implicit_supported(taps, c, h, w, x_ld, n)
    for c in R.CASES:
        if c["kind"] in ("i3", "i1"):
            assert R.implicit_supported(c["kh"] * c["kw"], c["C"], c["H"], c["W"], c["x_ld"], c["N"]), c["id"]


def test_plan_driven_cases_take_the_route_the_predicates_say(lib):
    routes = {pol: set() for pol in REACHES}
    for c in R.CASES:
        if c["kind"] != "mirror":
            continue
        real, mine = plan_of(lib, c), R.plan_py(R.geom_fields(c), R.POLICIES[c["policy"]])
        assert real == mine, (c["id"], real, mine)
        if c["policy"] in routes:
            routes[c["policy"]].add(real["route"])
    for pol, want in REACHES.items():
        assert routes[pol] == want, (pol, routes[pol] ^ want)
    # the two plans the table was built around
    p = plan_of(lib, R.BY_ID["m-i3-inplace-empty-split"])
    assert (p["route"], p["splits"], p["mp"], p["seg"]) == ("implicit_inplace", 8, 40 * 64, 320) and 7 * 320 >= 33 * 64
    p = plan_of(lib, R.BY_ID["m-tn-plan-M1088"])
    assert (p["route"], p["splits"], p["mp"], p["seg"]) == ("tn", 8, 1536, 192)
    f = R.forced_plan(R.BY_ID["tn-M1088-S8"])
    assert (f["splits"], f["mp"], f["seg"]) == (8, 1536, 192)
    # the engines' policies are the ones the table names
    for name, eng in (("unet", 0), ("vae", 1)):
        pol = N.WgradPolicy()
        assert lib.ctta_wgrad_engine_policy(eng, pol) == 0
        assert (pol.implicit_target, pol.implicit_cap, pol.direct, pol.upsample_copy) == R.POLICIES[name]


def test_table_reaches_every_class(lib):
    have = set()
    for c in R.CASES:
        have |= R.classes(c, plan_of(lib, c) if c["kind"] == "mirror" else None)
    assert not (R.REQUIRED_CLASSES - have), sorted(R.REQUIRED_CLASSES - have)
    # the generic 3x3 kernel and its width-64 copy get the same edge classes
    strip = lambda k: {s.replace(k, "*") for s in have if s.startswith("i3:%s:" % k)}      # noqa: E731
    assert strip("generic") == strip("w64")
    # every kernel the launcher can pick is launched by some i3 / i1 case
    kernels = {R.implicit_kernel(c["kh"] * c["kw"], c["W"], nat) for c in R.CASES if c["kind"] in ("i3", "i1")
               for nat in ((False, True) if c["kind"] == "i3" else (False,))}
    assert kernels == {"generic<9,nat>", "generic<9,dyt>", "w64<nat>", "w64<dyt>", "generic<1>"}
    assert all(set(c["families"]) >= {"uniform", "offset"} for c in R.CASES)
    assert all("impulse" in c["families"] for c in R.CASES if c["kind"] == "i3")
    # size: M <= about 2200, C and N <= 264
    assert all(R.positions(c) <= 2200 and c["C"] <= 264 and c["N"] <= 264 for c in R.CASES)


def layer_class(route, taps, wi, S, seg, M, nb):
    """(route, taps, width, a whole split beyond M, per-sample columns).  The width stays in the class wherever a kernel sees
    it: the implicit kernels' patch and ctta_im2col_t's borders.  On the two tn routes it is dropped: ctta_wgrad_tn takes the
    flat (M, C) and (M, N) matrices and never learns how the M rows were laid out as an image."""
    return (route, taps, 0 if route.startswith("tn") else wi, any(s * seg >= M for s in range(S)), nb > 0)


def test_real_layers_are_inside_the_table_classes(lib):
    geom = [f for f, _ in N.WgradGeom._fields_]
    plan = [f for f, _ in N.WgradPlanInfo._fields_]
    with open(os.path.join(ROOT, "tests", "golden", "wgrad_plan_cases.json")) as f:
        rows = [(n, dict(zip(geom, g)), dict(zip(plan, r))) for n, _, g, r in json.load(f) if not n.startswith("g")]
    # (the n260_* lines probe the plan at n % 8 != 0: no launch takes such a dY -- ctta_transpose_bf16 and the in-place
    # kernels refuse it -- so they are no layer either)
    rows = [r for r in rows if r[1]["n"] % 8 == 0]
    assert len(rows) >= 100 and len({n.split("/")[0] for n, _, _ in rows}) >= 20
    real = {layer_class(R.ROUTES[p["route"]], g["kh"] * g["kw"], g["wi"], p["splits"], p["seg"], g["batch"] * g["ho"] * g["wo"], g["nb"])
            for _, g, p in rows}
    mine = set()
    for c in R.CASES:
        if c["kind"] == "rowsum":
            continue
        M, taps = R.positions(c), c["kh"] * c["kw"]
        if c["kind"] == "mirror":
            p = plan_of(lib, c)
            mine.add(layer_class(p["route"], taps, R.out_hw(c)[1], p["splits"], p["seg"], M, c["nb"]))
            continue
        p = R.forced_plan(c)
        forms = {"i3": ("implicit_dyt", "implicit_inplace"), "tn": ("tn",), "i1": ()}[c["kind"]]
        for r in forms:
            mine.add(layer_class(r, taps, c["W"], p["splits"], p["seg"], M, c["nb"]))
        if c["kind"] in ("i3", "tn"):            # the direct form of the same geometry: one split, no per-sample columns
            mine.add(layer_class("implicit_direct" if c["kind"] == "i3" else "tn_direct", taps, c["W"], 1, R.rup(M, 64), M, 0))
    assert real <= mine, sorted(real - mine)
