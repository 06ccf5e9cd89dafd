"""tests/conv_ref.py on the CPU: the float64 reference against F.conv2d and autograd, what the input families promise, the
two conditions that make the `integer` / `impulse` families bit-exact, the mirror of the per-wave epilogue choice, and the
COVERAGE of the case table -- proved from the plan ctta_conv_plan gives every case (test_conv_plan_cpu.py's ENV0), not from
the case names: every tile id, every gather / schedule / epilogue class with the plan fields that define it, and elements on
both wave routes wherever both can occur.  Every class check counts its cases, so an emptied list fails."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
from consistencytta_amd import _native as N


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


@pytest.fixture(scope="module")
def plans(lib):
    """id -> (status, plan or error text)"""
    return {c["id"]: R.plan(lib, c) for c in R.CASES}


def _routes(lib, c, pl):
    g = R.tile_geom(lib, pl["variant"]) if pl["variant"] else None
    tg = R.tile_geom(lib, pl["tail_variant"]) if pl["tail_variant"] else None
    r = R.wave_routes(c, pl, g, tg)
    return {R.ROUTES[i] for i in r.unique().tolist()}


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("kw", [dict(kh=3, kw=3, ph=1, pw=1), dict(kh=3, kw=3), dict(kh=3, kw=3, ph=1, pw=1, sh=2, sw=2),
                                dict(kh=1, kw=5, pw=6, dw=3), dict(kh=3, kw=2, ph=2, pw=1, dh=2, sw=2), dict(kh=3, kw=3, ph=1, pw=1, ups=1),
                                dict(kh=3, kw=3, ph=1, pw=1, c1=16), dict(kh=5, kw=5, ph=2, pw=2, ups=1)])
def test_reference_equals_conv2d_in_float64(kw):
    c = R._case("ref", [], B=2, hs=5, ws=6, c0=8, n=12, **kw)
    inp = R.make_inputs(c, "uniform")
    ref = R.reference(c, inp, "uniform")
    x = inp["x"][0].double() if inp["x1"] is None else torch.cat([inp["x"][0].double(), inp["x1"].double()], -1)
    xn = x.permute(0, 3, 1, 2)
    if c["ups"]:
        xn = F.interpolate(xn, scale_factor=2.0, mode="nearest")
    w = inp["w"][0].double().view(c["n"], c["kh"], c["kw"], c["ct"]).permute(0, 3, 1, 2)
    y = F.conv2d(xn, w, None, stride=(c["sh"], c["sw"]), padding=(c["ph"], c["pw"]), dilation=(c["dh"], c["dw"]))
    assert y.shape[2:] == (c["ho"], c["wo"])
    got = ref["sum"][0].view(c["B"], c["ho"], c["wo"], c["n"]).permute(0, 3, 1, 2)
    assert float((got - y).abs().max()) < 1e-10
    ya = F.conv2d(xn.abs(), w.abs(), None, stride=(c["sh"], c["sw"]), padding=(c["ph"], c["pw"]), dilation=(c["dh"], c["dw"]))
    assert float((ref["A"][0].view(c["B"], c["ho"], c["wo"], c["n"]).permute(0, 3, 1, 2) - ya).abs().max()) < 1e-10


@pytest.mark.parametrize("k,pad", [(3, 0), (3, 1), (4, 1)])
def test_reference_in_the_data_gradient_form_equals_autograd(k, pad):
    """The data gradient of y = conv2d(x, w, padding = pad) is the convolution of dy with the taps reversed and (cin, cout)
    swapped at padding k - 1 - pad: the `3x3-pad2-dgrad` class of the table."""
    B, cin, cout, H, W = 2, 8, 16, 6, 5
    x = R.det("dg.x", (B, cin, H, W), 1).double().requires_grad_(True)
    w = R.det("dg.w", (cout, cin, k, k), 2).double()
    y = F.conv2d(x, w, None, padding=pad)
    dy = R.det("dg.dy", tuple(y.shape), 3).double()
    y.backward(dy)
    c = R._case("dgrad", [], B=B, hs=y.shape[2], ws=y.shape[3], c0=cout, n=cin, kh=k, kw=k, ph=k - 1 - pad, pw=k - 1 - pad)
    assert (c["ho"], c["wo"]) == (H, W)
    wd = w.flip(2, 3).permute(1, 2, 3, 0).reshape(1, cin, k * k * cout)           # [cin][(kh, kw, cout)]
    inp = dict(x=dy.permute(0, 2, 3, 1).unsqueeze(0), x1=None, w=wd)
    got = R.reference(c, inp, "uniform")["sum"][0].view(B, H, W, cin).permute(0, 3, 1, 2)
    assert float((got - x.grad).abs().max()) < 1e-10


def test_reference_epilogue_order_and_outputs():
    c = R._case("epi", [], B=2, hs=3, ws=3, c0=8, n=8, bias=1, rowvec=1, res=1, bias_m=1, acc=1, alpha=1, out_act=3, out2=1)
    for fam in ("uniform", "integer"):
        inp, s = R.make_inputs(c, fam), R.slopes(fam)
        ref = R.reference(c, inp, fam)
        b = torch.arange(c["M"]) // 9
        tot = s["alpha"] * (ref["sum"][0] + inp["bias"].double() + inp["rowvec"].double()[b] + inp["bias_m"].double().view(-1, 1) +
                            inp["res"].double() + inp["old"].double())
        assert torch.equal(tot, ref["tot"][0])
        assert torch.equal(ref["val"][0], torch.where(tot > 0, tot, tot * s["out_slope"]))
        out, out2 = R.expected_out(c, ref, fam)
        assert torch.equal(out, R.bf16_round(out)) and torch.equal(out2, R.bf16_round(F.leaky_relu(out, s["out2_slope"])))
        assert bool((ref["A"] >= ref["tot"].abs() - 1e-12).all())


def test_geglu_reference_uses_the_packing_of_the_existing_test():
    hid, k, rows = 48, 16, 5
    w, b, x = R.det("gg.w", (2 * hid, k), 1), R.det("gg.b", (2 * hid,), 2), R.det("gg.x", (rows, k), 3)
    proj = F.linear(x.double(), w.double(), b.double())
    want = proj[:, :hid] * F.gelu(proj[:, hid:])
    wi, bi = torch.zeros(2 * hid, k), torch.zeros(2 * hid)
    for j in range(hid):          # test_linear_with_fused_geglu_epilogue
        wi[(j // 16) * 32 + j % 16], wi[(j // 16) * 32 + 16 + j % 16] = w[j], w[hid + j]
        bi[(j // 16) * 32 + j % 16], bi[(j // 16) * 32 + 16 + j % 16] = b[j], b[hid + j]
    c = R._case("gg", [], B=1, hs=rows, ws=1, c0=k, n=2 * hid, out_act=4, bias=1)
    ref = R.reference(c, dict(x=x.view(1, 1, rows, 1, k), x1=None, w=wi.unsqueeze(0), bias=bi), "uniform")
    assert float((ref["val"][0] - want).abs().max()) < 1e-12


def test_dest_index_is_the_remap_of_the_conv_transpose_test():
    """out[b][l][o], l = q * u + r - pad: row q of the GEMM holds u output positions x Cout (test_conv_transpose1d_as_phase_gemm)."""
    c = R.BY_ID["e-str-t21"]
    st, co, u = c["strided"], 24, 4
    Lout, pad, Q = st["lim"] // co, -st["off"] // co, c["wo"]
    idx = R.dest_index(c)[0]
    seen = torch.zeros(c["B"] * st["obs"], dtype=torch.int64)
    for m in (0, 1, Q - 1, Q, c["M"] - 1):
        b, q = divmod(m, Q)
        for j in (0, 23, 24, 47, 48, 95):
            r, o = divmod(j, co)
            l = q * u + r - pad
            assert int(idx[m, j]) == ((b * Lout + l) * co + o if 0 <= l < Lout else -1), (m, j)
    v = idx[idx >= 0]
    seen[v] += 1
    assert bool((seen == 1).all())                                   # every output element is written exactly once
    assert int(idx[0, 0]) == -1 and int(idx[Q - 1, 95]) == -1        # both ends of a sample are clipped


# ------------------------------------------------------------------------------------------------ the generators
def test_families_give_what_they_promise():
    c = R._case("fam", [], B=3, hs=4, ws=5, c0=16, c1=8, n=8, kh=3, kw=3, ph=1, pw=1, bias=1, rowvec=1, res=1)
    u, o, i = (R.make_inputs(c, f) for f in ("uniform", "offset", "integer"))
    for inp in (u, o, i):
        for k in ("x", "x1", "w", "res", "old"):
            assert torch.equal(inp[k], R.bf16_round(inp[k])), k
    assert float(u["x"].mean().abs()) < 0.1 and float(o["x"].min()) > 0 and float(o["w"].min()) > 0
    gaps = (u["rowvec"][1:] - u["rowvec"][:-1]).abs()
    assert float(gaps.min()) >= 1.0 - 1e-6                       # a neighbour's row vector is O(1) away on EVERY channel
    assert set(i["x"].unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and set(i["w"].unique().tolist()) <= {-1.0, 0.0, 1.0}
    for k in ("bias", "rowvec", "res", "old", "bias_m"):
        assert torch.equal(i[k], i[k].round()) and float(i[k].abs().max()) <= 12
    gi = (i["rowvec"][1:] - i["rowvec"][:-1]).abs()
    assert float(gi.min()) >= 1.0
    for fam in ("uniform", "integer"):
        s = R.slopes(fam)
        assert all(v == float(np.float32(v)) for v in s.values())
    si = R.slopes("integer")
    assert all(np.log2(v) == round(np.log2(v)) for v in si.values())
    assert (R.slopes("uniform")["in_slope"], R.slopes("uniform")["out_slope"]) == (R.f32(0.1), R.f32(0.01))
    p = R.make_inputs(R._case("imp", [], B=2, hs=4, ws=5, c0=16, c1=8, n=8, kh=3, kw=3, ph=1, pw=1), "impulse")
    assert set(p["x"].unique().tolist()) == {0.0, 1.0} and 1 <= int(p["x"].sum() + p["x1"].sum()) <= 7
    assert int(p["x1"].sum()) >= 1                                 # an impulse on each side of the source boundary
    assert float(p["bias"].abs().max()) == 0.0
    # thinning: the share of nonzero w follows 576 / K
    big = R.make_inputs(R._case("thin", [], B=1, hs=2, ws=2, c0=256, n=64, kh=3, kw=3, ph=1, pw=1), "integer")
    share = float((big["w"] != 0).float().mean())
    assert abs(share - (2.0 / 3.0) * 0.25) < 0.02                  # round(1.49 u) != 0 for 2/3 of the draws, K = 2304: 1/4 kept


@pytest.mark.parametrize("case,family", [(c, f) for c, f in R.case_params() if f in ("integer", "impulse")],
                         ids=["%s-%s" % (c["id"], f) for c, f in R.case_params() if f in ("integer", "impulse")])
def test_integer_and_impulse_cases_are_exact_in_fp32_and_bf16(lib, case, family):
    """sum |x| |w| + |epilogue terms| < 2^24: every fp32 partial sum, in any order, split or not, is an exactly represented
    integer (multiple of 2^-k after the power-of-two scale); and the value is a bf16 number: one right answer, bit for bit."""
    inp = R.make_inputs(case, family)
    ref = R.reference(case, inp, family)
    s = R.slopes(family)
    alpha = s["alpha"] if case["alpha"] else 1.0
    q = 2.0 if case["in_act"] else 1.0                    # bf16(leaky(x, 1/2)) of an integer: halves
    assert float(ref["A"].max()) / alpha * q < 2.0 ** 24
    assert torch.equal(ref["sum"] * q, (ref["sum"] * q).round())
    val = ref["val"]
    assert torch.equal(val.float().double(), val)
    if case["gn"]:          # integers + 1/64: the sums of the contract are exact in fp32, the stored bf16 numbers are other numbers
        pl = R.plan(lib, case, family)[1]
        _, a1, _ = R.gn_reference(case, ref, pl, R.tile_geom(lib, pl["variant"]))
        q = 64 / (alpha * s["out_slope"] if case["out_act"] == 3 else alpha)          # the values are multiples of 1 / q
        assert q * float(a1.max()) < 2.0 ** 24 and torch.equal(val * q, (val * q).round())
        assert float((R.bf16_round(val.float()).double() != val).double().mean()) > 0.5
    else:
        assert torch.equal(R.bf16_round(val.float()).double(), val), float(val.abs().max())
    if case["out2"]:
        v2 = torch.where(val > 0, val, val * s["out2_slope"])
        assert torch.equal(R.bf16_round(v2.float()).double(), v2)
    if family == "impulse":
        assert float(ref["val"].abs().max()) > 0          # the impulses reach the output


def test_bound_holds_for_a_chained_fp32_emulation():
    """Blocks of 8 products summed one term at a time in fp32, the block sums chained in fp32, then the epilogue in the
    kernel's order: the emulation must sit inside the bound, and well inside it."""
    c = R._case("emu", [], B=2, hs=6, ws=5, c0=64, n=16, kh=3, kw=3, ph=1, pw=1, bias=1, rowvec=1, res=1)
    for fam in ("uniform", "offset"):
        inp = R.make_inputs(c, fam)
        ref = R.reference(c, inp, fam)
        q = R.gather64(c, inp["x"][0], None).numpy().astype(np.float32)
        w = inp["w"][0].numpy().astype(np.float32)
        acc = np.zeros((c["M"], c["n"]), np.float32)
        for k0 in range(0, c["K"], 8):
            blk = np.zeros_like(acc)
            for k in range(k0, k0 + 8):
                blk = blk + q[:, k:k + 1] * w[:, k][None, :]
            acc = acc + blk
        b = np.arange(c["M"]) // 30
        v = acc + (inp["bias"].numpy()[None, :] + inp["rowvec"].numpy()[b])
        v = v + inp["res"].numpy()
        got = torch.from_numpy(v).to(torch.bfloat16).double()
        pl = dict(splits=1, kind=0)
        r = R.worst_ratio((got - ref["val"][0]).abs(), R.bound(c, ref, pl)[0])
        assert r < 1.0, (fam, r)


# ------------------------------------------------------------------------------------------------ the route mirror
def test_wave_routes_mirror_on_a_hand_worked_launch():
    """64x64 tile of 2 x 2 waves (TM = TN = 32), M = 100 = 2 samples of 50 rows, n = 40, rowvec: tile 0 (rows 0..63) straddles
    the samples -> generic code everywhere; tile 1 (rows 64..99) lies in sample 1 -> straight-line for columns 0..31, the
    column-edge wave (32..39) generic."""
    c = R._case("rt", [], B=2, hs=50, ws=1, c0=64, n=40, bias=1, rowvec=1)
    g = dict(bm=64, bn=64, tm=32, tn=32)
    pl = dict(halo=0, splits=1, kind=0, wide_f32=0, wide_store=1, epi_fast=1, epi_fast_geglu=0, plain_out=1, tail_rows=0)
    r = R.wave_routes(c, pl, g)
    name = lambda m, j: R.ROUTES[int(r[m, j])]          # noqa: E731
    assert name(0, 0) == "wide4_sample" and name(63, 31) == "wide4_sample" and name(10, 35) == "wide4_edge"
    assert name(64, 0) == "fast" and name(99, 31) == "fast" and name(64, 32) == "wide4_edge"
    c2 = dict(c, rowvec=0)
    assert R.ROUTES[int(R.wave_routes(c2, pl, g)[0, 0])] == "fast"
    # strided destination: the WAVE's rows decide -- rows 32..63 hold the boundary at 50
    r3 = R.wave_routes(c2, dict(pl, plain_out=0), g)
    assert [R.ROUTES[int(r3[m, 0])] for m in (0, 31, 32, 63, 64, 99)] == ["fast_str", "fast_str", "wide4_str", "wide4_str", "fast_str", "fast_str"]
    assert R.ROUTES[int(R.wave_routes(c2, dict(pl, epi_fast=0), g)[0, 0])] == "wide4"
    assert R.ROUTES[int(R.wave_routes(c2, dict(pl, splits=4), g)[0, 0])] == "finish_wide4"


def test_tile_geometry_comes_from_the_variant_names(lib):
    assert lib.ctta_conv_gemm_num_variants() == 43
    g = R.tile_geom(lib, 29)
    assert (g["bm"], g["bn"], g["bk"], g["wm"], g["wn"], g["mode"], g["stages"], g["sk"], g["tm"], g["tn"], g["frags"]) == \
           (256, 256, 64, 2, 4, 2, 2, False, 128, 64, 32)
    assert R.tile_geom(lib, 41)["sk"] and R.tile_geom(lib, 4)["tn"] == 32 and R.tile_geom(lib, 21)["frags"] == 4
    assert [R.tile_geom(lib, t)["mode"] for t in R.GATHER_TILES] == [0, 1, 2]
    assert tuple(t for t in range(1, 44) if R.tile_geom(lib, t)["mode"] == 2) == R.MODE2_IDS
    assert tuple(t for t in range(1, 44) if R.tile_geom(lib, t)["bk"] == 32) == R.BK32_IDS
    assert [R.tile_geom(lib, t)["frags"] for t in R.EPI_TILES] == [4, 16, 32] and R.tile_geom(lib, 29)["wm"] * R.tile_geom(lib, 29)["wn"] == 8


# ------------------------------------------------------------------------------------------------ coverage, from the plans
def test_every_case_plans_or_is_refused_as_the_table_says(plans):
    n_run = n_ref = 0
    for c in R.CASES:
        st, pl = plans[c["id"]]
        if c.get("refused"):
            assert st != 0 and c["refused"] in pl, (c["id"], pl)
            n_ref += 1
        else:
            assert st == 0, (c["id"], pl)
            assert c["tile"] == 0 or pl["variant"] == c["tile"] or pl["halo"]
            for f in c["families"]:          # the plan does not depend on the family (alpha and the slopes stay in their classes)
                assert R.plan(N.lib(), c, f) == (st, pl), c["id"]
            n_run += 1
    assert n_run >= 240 and n_ref >= 7


def test_all_43_tile_ids_run_ragged_in_m_and_n(lib, plans):
    seen = {}
    for c in R.CASES:
        if "tile" not in c["cls"]:
            continue
        st, pl = plans[c["id"]]
        g = R.tile_geom(lib, c["tile"])
        assert st == 0 and pl["variant"] == c["tile"]
        if not g["sk"]:
            assert c["M"] % g["bm"] != 0 and c["n"] % g["tn"] != 0 and c["ldc"] > c["n"], c["id"]
            if c["rowvec"]:
                assert {"fast", "wide4_edge"} <= _routes(lib, c, pl), c["id"]
        if "tile:c40" in c["cls"]:
            assert c["ct"] % g["bk"] != 0 and c["c1"] == 0          # a K tile straddles taps
        if "tile:concat" in c["cls"]:
            assert c["c1"] > 0 and c["c0"] % g["bk"] != 0 or c["c0"] % g["bk"] == 0 and c["ct"] % g["bk"] != 0
        if "tile:ct%bk==0" in c["cls"]:
            assert g["mode"] == 2 and c["ct"] % g["bk"] == 0
        if "tile:bk32:c96" in c["cls"]:
            assert g["bk"] == 32 and c["c0"] == 96 and c["c0"] % 64 != 0
        for k in c["cls"]:
            seen.setdefault(k, set()).add(c["tile"])
    assert seen["tile"] == set(range(1, 44))
    assert seen["tile:c40"] >= set(range(1, 17)) and seen["tile:concat"] >= set(range(1, 17))
    assert seen["tile:ct%bk==0"] == set(R.MODE2_IDS) - set(R.SK_IDS)
    assert seen["tile:bk32:c96"] == set(R.BK32_IDS)
    assert seen["tile:sk:M768"] == set(R.SK_IDS) and seen["tile:sk:M2560"] == set(R.SK_IDS)
    assert {c["M"] for c in R.CASES if "tile:sk:M768" in c["cls"]} == {768} and {c["M"] for c in R.CASES if "tile:sk:M2560" in c["cls"]} == {2560}
    # the staging twins that must be bit-equal run on the same inputs
    for i in range(1, 9):
        for sfx in ("c40", "cat"):
            a, b = R.BY_ID["t%d-%s" % (i, sfx)], R.BY_ID["t%d-%s" % (i + 8, sfx)]
            assert {k: v for k, v in a.items() if k not in ("id", "tile")} == {k: v for k, v in b.items() if k not in ("id", "tile")}


GATHER_CLASSES = {
    "3x3-pad1": lambda c: (c["kh"], c["kw"], c["ph"], c["pw"], c["sh"], c["dh"], c["ups"]) == (3, 3, 1, 1, 1, 1, 0),
    "3x3-pad0": lambda c: (c["kh"], c["kw"], c["ph"], c["pw"]) == (3, 3, 0, 0) and c["ho"] == c["hi"] - 2,
    "3x3-pad2-dgrad": lambda c: (c["kh"], c["ph"], c["pw"]) == (3, 2, 2) and c["ho"] == c["hi"] + 2,
    "stride2": lambda c: (c["sh"], c["sw"]) == (2, 2) and c["kh"] == 3,
    "1xk-dil3": lambda c: c["kh"] == 1 and c["dw"] == 3 and c["kw"] > 1 and c["wo"] == c["wi"],
    "1xk-dil5": lambda c: c["kh"] == 1 and c["dw"] == 5 and c["kw"] > 1 and c["wo"] == c["wi"],
    "1x1": lambda c: c["kh"] * c["kw"] == 1 and c["groups"] == 1,
    "1x16": lambda c: (c["kh"], c["kw"]) == (1, 16),
    "1x32": lambda c: (c["kh"], c["kw"]) == (1, 32),
    "ups3x3": lambda c: c["ups"] == 1 and (c["kh"], c["kw"], c["ph"]) == (3, 3, 1) and c["ho"] == 2 * c["hs"],
    "width1": lambda c: c["wi"] == 1 and c["kw"] == 3 and c["pw"] == 1,
    "width2": lambda c: c["wi"] == 2 and c["kw"] == 3 and c["pw"] == 1,
    "width3": lambda c: c["wi"] == 3 and c["kw"] == 3 and c["pw"] == 1,
    "wo1": lambda c: c["wo"] == 1 and c["ho"] > 1,
    "howo1": lambda c: c["ho"] * c["wo"] == 1 and c["M"] > 64,
    "x_stride": lambda c: c["xs"] > c["c0"] and c["groups"] == 1,
    "groups3": lambda c: c["groups"] == 3 and c["xgs"] > 0 and c["wgs"] > 0 and c["ogs"] > c["M"] * c["ldc"],
    "in_act": lambda c: c["in_act"] == 1,
}
GATHER_REFUSED_BY_MODE2 = {
    "concat": lambda c: c["c1"] > 0,
    "c40": lambda c: c["ct"] % 64 != 0,
    "1x33": lambda c: c["kh"] * c["kw"] == 33,
    "ups5x5": lambda c: c["ups"] == 1 and c["kh"] == 5,
}


def test_gather_classes_run_on_every_staging_mode_that_admits_them(lib, plans):
    count = 0
    for name, pred in list(GATHER_CLASSES.items()) + list(GATHER_REFUSED_BY_MODE2.items()):
        for mode, t in enumerate(R.GATHER_TILES):
            c = R.BY_ID["g-%s-m%d" % (name, mode)]
            st, pl = plans[c["id"]]
            assert pred(c) and c["tile"] == t and "gather:%s" % name in c["cls"], c["id"]
            assert c["n"] % R.tile_geom(lib, t)["tn"] != 0          # a column-edge wave in every launch
            if name in GATHER_REFUSED_BY_MODE2 and mode == 2:
                assert st != 0 and "needs (c0+c1) % BK == 0" in pl
            elif name == "in_act" and mode > 0:
                assert st != 0 and "in_act needs a register-staged variant" in pl
            else:
                assert st == 0 and pl["variant"] == t and R.tile_geom(lib, t)["mode"] == mode, (c["id"], pl)
                assert "integer" in c["families"] and "uniform" in c["families"]
                count += 1
    assert count == 3 * len(GATHER_CLASSES) - 2 + 2 * len(GATHER_REFUSED_BY_MODE2)


SCHEDULE_CLASSES = {
    "sched:xcd:n_inner=1": lambda c, p: p["xcd_per"] > 0 and p["n_inner"] == 1 and p["m_tiles"] % 8 == 0,
    "sched:xcd:n_inner=0": lambda c, p: p["xcd_per"] > 0 and p["n_inner"] == 0 and p["n_tiles"] > 4,
    "sched:xcd:padding": lambda c, p: p["xcd_per"] > 0 and 8 * p["xcd_per"] > p["m_tiles"],
    "sched:slab": lambda c, p: p["slab_total"] > 0 and p["splits"] == 1 and 8 * p["slab_per"] > p["slab_total"],
    "sched:splitk": lambda c, p: p["splits"] > 1 and p["finish_blocks"] > 0,
    "sched:splitk:full": lambda c, p: p["splits"] > 1 and p["wide_store"] == 1 and c["rowvec"] and c["res"] and c["out2"] and p["epi_act"],
    "sched:splitk:f32": lambda c, p: p["splits"] > 1 and c["out_f32"] == 1 and p["prof_code"] == p["variant"] + 100,
    "sched:splitk:not-wide-f32": lambda c, p: p["splits"] > 1 and p["splitk_wide_f32"] == 0,
    "sched:splitk:nk%splits": lambda c, p: p["splits"] > 1 and p["nk"] % p["splits"] != 0 and p["nk"] % p["nk_split"] != 0,
    "sched:streamk": lambda c, p: p["kind"] == 2 and p["grid_x"] > 1,
    "sched:halo": lambda c, p: p["halo"] == 1 and c["c0"] == 32 and c["n"] == 32 and c["dw"] == 3,
    "sched:tail": lambda c, p: p["tail_rows"] == 32 and p["variant"] == 29 and p["tail_variant"] == 21 and c["tile"] == 0,
}


def test_schedule_classes_are_what_the_plan_says(plans):
    counts = dict.fromkeys(SCHEDULE_CLASSES, 0)
    for c in R.CASES:
        for k in c["cls"]:
            if k in SCHEDULE_CLASSES:
                st, pl = plans[c["id"]]
                assert st == 0 and SCHEDULE_CLASSES[k](c, pl), (c["id"], k, pl)
                counts[k] += 1
    assert all(v >= 1 for v in counts.values()), counts
    assert {c["tile"] for c in R.CASES if "sched:splitk:not-wide-f32" in c["cls"]} == {10, 18}
    # stream-K: a tile folded by three workgroups, and whole (unsplit) tiles beside split ones
    parts = {c["id"]: R.sk_max_parts(plans[c["id"]][1]) for c in R.CASES if "sched:streamk" in c["cls"]}
    assert max(parts.values()) >= 3 and min(parts.values()) >= 2, parts
    assert sum(1 for c in R.CASES if "sched:streamk" in c["cls"] and c["ws_bind"]) == len(parts)


EPI_FAST = ("bias", "rowvec", "res", "res+out2", "acc")
EPILOGUE_CLASSES = {
    "bias": lambda c, p: c["bias"] and not (c["rowvec"] or c["res"] or c["acc"] or c["out2"]) and p["epi_fast"] and not p["epi_act"],
    "rowvec": lambda c, p: c["rowvec"] and p["epi_fast"] and not p["epi_act"],
    "res": lambda c, p: c["res"] and not c["out2"] and p["epi_fast"] and not p["epi_act"],
    "res+out2": lambda c, p: c["res"] and c["out2"] and p["epi_fast"] and not p["epi_act"],
    "acc": lambda c, p: c["acc"] and not c["res"] and p["epi_fast"] and not p["epi_act"],
    "acc+res+lrelu+alpha": lambda c, p: c["acc"] and c["res"] and c["out_act"] == 3 and c["alpha"] and p["epi_fast"] and p["epi_act"],
    "bias_m": lambda c, p: c["bias_m"] and p["wide_store"] and not p["epi_fast"],
    "silu": lambda c, p: c["out_act"] == 1 and p["wide_store"] and not p["epi_fast"],
    "tanh": lambda c, p: c["out_act"] == 2 and p["wide_store"] and not p["epi_fast"],
    "f32-wide": lambda c, p: c["out_f32"] and p["wide_f32"] == 1,
    "f32-not-wide": lambda c, p: c["out_f32"] and p["wide_f32"] == 0 and not p["wide_store"],
    "scalar-ldc1": lambda c, p: c["ldc"] == 1 and c["n"] == 1 and c["out_f32"] and c["out_act"] == 2,
    "scalar-ldc3": lambda c, p: c["ldc"] == 3 and c["n"] == 3 and not c["out_f32"],
    "plain-n%4": lambda c, p: c["n"] % 4 != 0 and R.rup(c["n"], 4) <= c["ldc"] and c["ldc"] % 4 == 0 and not p["wide_store"],
    "str": lambda c, p: not p["plain_out"] and p["epi_fast"] and not p["epi_act"] and not c["out2"],
    "str+out2+lrelu": lambda c, p: not p["plain_out"] and p["epi_fast"] and p["epi_act"] and c["out2"],
}


def test_epilogue_classes_run_on_one_tile_of_each_epilogue_shape(lib, plans):
    counts = dict.fromkeys(EPILOGUE_CLASSES, 0)
    for name, pred in EPILOGUE_CLASSES.items():
        for t in R.EPI_TILES:
            c = R.BY_ID["e-%s-t%d" % (name, t)]
            st, pl = plans[c["id"]]
            assert st == 0 and pl["variant"] == t and pl["splits"] == 1 and pred(c, pl), (c["id"], pl)
            routes = _routes(lib, c, pl)
            if name in EPI_FAST or name == "acc+res+lrelu+alpha":          # both wave routes in one launch
                assert {"fast", "wide4_edge"} <= routes, (c["id"], routes)
            if name == "rowvec":          # a tile inside one sample and one that straddles two
                assert "wide4_sample" in routes and c["M"] // c["B"] % R.tile_geom(lib, t)["bm"] != 0
            if name.startswith("str"):
                idx = R.dest_index(c)[0]
                q = c["ho"] * c["wo"]
                assert {"fast_str", "wide4_str"} <= routes and int(idx[0, 0]) == -1 and int(idx[q - 1, -1]) == -1 and int(idx[q, 0]) == -1
            if name in ("bias_m", "silu", "tanh"):
                assert routes == {"wide4"}
            if name.startswith("scalar") or name in ("plain-n%4", "f32-not-wide"):
                assert routes == {"store"}
            counts[name] += 1
    assert all(v == len(R.EPI_TILES) for v in counts.values()), counts


def test_geglu_and_groupnorm_cases(lib, plans):
    # fused GEGLU, direct form (epilogue_geglu in the MFMA layout): one sample with an out_batch_stride of its own is not a plain
    # destination, so the wide store is off; the <= 8-fragment tiles carry it, the rules pick 64x128x64 for it
    direct = set()
    for c in (k for k in R.CASES if "epi:geglu-direct" in k["cls"]):
        st, pl = plans[c["id"]]
        if c.get("refused"):
            assert st != 0 and c["refused"] in pl and R.tile_geom(lib, c["tile"])["frags"] > 8
            direct.add("refused")
            continue
        g = R.tile_geom(lib, pl["variant"])
        assert st == 0 and pl["wide_store"] == 0 and pl["plain_out"] == 0 and pl["epi_fast_geglu"] == 0 and g["frags"] <= 8
        assert c["strided"]["obs"] != c["ho"] * c["wo"] * c["ldc"] and c["M"] % g["bm"] != 0 and c["ho"] * c["wo"] % g["tm"] != 0
        direct.add("B%d" % c["B"])
        assert _routes(lib, c, pl) == {"geglu_direct"} and (c["tile"] or pl["variant"] == 22)
        direct.add((g["bm"], g["bn"], g["mode"]))
    assert direct >= {(64, 64, 0), (64, 64, 2), (64, 128, 2), (128, 64, 2), (256, 32, 2), "refused", "B1", "B2"}
    assert sum(1 for c in R.CASES if "epi:geglu-direct" in c["cls"] and c["n"] % R.tile_geom(lib, c["tile"] or 22)["bn"] != 0) >= 5
    # wide-store forms: the straight-line one and, on the TN = 64 tiles, a column-edge wave through the rolled one
    seen = set()
    for c in (k for k in R.CASES if "epi:geglu" in k["cls"]):
        st, pl = plans[c["id"]]
        if c.get("refused"):
            assert st != 0 and R.tile_geom(lib, c["tile"])["frags"] == 32
            seen.add("refused")
            continue
        assert st == 0 and pl["epi_fast_geglu"] == 1 and pl["wide_store"] == 1 and R.tile_geom(lib, c["tile"])["frags"] <= 16
        seen |= _routes(lib, c, pl)
        seen.add("waves%d" % (R.tile_geom(lib, c["tile"])["wm"] * R.tile_geom(lib, c["tile"])["wn"]))
    assert {"geglu_fast", "geglu_wide4", "refused", "waves4", "waves8"} <= seen
    n = {"below": 0, "equal": 0, "above": 0, "edge": 0, "act": 0, "res0": 0, "res1": 0}
    for c in (k for k in R.CASES if "epi:gn" in k["cls"]):
        st, pl = plans[c["id"]]
        g = R.tile_geom(lib, c["tile"])
        cpg = c["n"] // c["gn"]
        cw = min(cpg, g["tn"])
        assert st == 0 and pl["gn_nchunk"] == (c["ho"] * c["wo"]) // g["bm"] * g["wm"] * (cpg // cw)
        assert pl["epi_fast"] == (0 if "epi:gn:act" in c["cls"] else 1)
        rel = "below" if cpg < g["tn"] else "equal" if cpg == g["tn"] else "above"
        if "epi:gn:act" in c["cls"]:          # alpha and a LeakyReLU: no statistics instantiation, every wave sums in epilogue_wide4
            assert pl["epi_act"] == 1 and c["alpha"] and c["out_act"] == 3 and _routes(lib, c, pl) == {"wide4"}
            n["act"] += 1
        elif "epi:gn:column-edge" in c["cls"]:
            assert {"fast", "wide4_edge"} <= _routes(lib, c, pl)
            n["edge"] += 1
        else:
            assert "epi:gn:cpg-%s" % rel in c["cls"] and _routes(lib, c, pl) == {"fast"}
            n[rel] += 1
        n["res%d" % c["res"]] += 1
    assert all(v >= 1 for v in n.values()) and n["below"] == n["equal"] == n["above"] == 6, n
