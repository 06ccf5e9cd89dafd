"""conv_gemm forward, every tile, gather, schedule and epilogue route of tests/conv_ref.py's table, per element.

Each (case, input family) is one ctta_conv_gemm call on poisoned buffers:
  NaN guard bands directly before and behind the x, second-source and residual allocations, NaN in the x columns
  [c0, x_stride), in the residual / row-vector columns behind n, in the weight rows behind n of the same allocation; the K
  columns [K, k_pad) of the weights are zero (the contract of ctta_conv_desc.w);
  every output (out, out2, the GroupNorm partials) starts as a finite sentinel with sentinel guard bands around it.
Asserted:
  every valid element was written and is finite; every other element of the output allocations -- columns [n, ldc), rows behind
  M, the positions out_limit clips, the guard bands -- keeps the sentinel bit for bit (one exception, asserted too: with n % 4
  != 0 the plain epilogue stores whole groups of four channels, so columns [n, round_up(n, 4)) hold 0.0);
  `uniform` / `offset`: |stored - float64 reference| <= the per-element bound of conv_ref.py, for every element, and the worst
  error / bound is kept per epilogue code (conv_ref.wave_routes) for the report at the end of the file;
  `integer` / `impulse`: the stored values ARE the reference, on every route (two-pass split-K, stream-K and both K orders
  included);  out2 = bf16(leaky(out as stored));
  GroupNorm partials: ctta_conv_last_gn_chunks() == the plan's gn_nchunk and every (sample, chunk, group) entry within its own
  bound of the float64 sums of the values BEFORE the bf16 rounding (the contract include/ctta.h states); on `integer`, where
  these cases draw integers + 1/64, the sums equal the float64 ones exactly.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_ref as R  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402

DEV = "cuda:0"
GUARD = 256
WORST = {}            # (route, family) -> worst error / bound, for test_report


def lib():
    return N.lib()


@pytest.fixture(scope="module")
def workspace():
    """A stream-K workspace with a zeroed header, as test_streamk_fold_is_exact_ordered_and_repeatable binds it."""
    ws = torch.zeros(lib().ctta_conv_workspace_bytes(), dtype=torch.uint8, device=DEV)
    # The labels, L and the schedule classes come from ctta_conv_plan under conv_ref.ENV0; ctta_conv_gemm plans from the live
    # process.  The two must describe the same machine, or a split-K case would quietly test an unsplit launch.
    bound, nbytes = ctypes.c_void_p(), ctypes.c_size_t()
    lib().ctta_conv_bound_workspace(ctypes.byref(bound), ctypes.byref(nbytes))
    live = dict(cu_count=torch.cuda.get_device_properties(0).multi_processor_count, xcd=N.get_option("xcd"),
                splitk=N.get_option("splitk"), streamk=N.get_option("streamk"), streamk_grid=N.get_option("streamk_grid"),
                workspace_bytes=lib().ctta_conv_workspace_bytes(), bound_workspace=bound.value)
    want = dict({k: R.ENV0[k] for k in ("cu_count", "xcd", "splitk", "streamk", "streamk_grid", "workspace_bytes")}, bound_workspace=None)
    assert live == want, "the live process is not the environment the table was planned under: %r" % live
    yield ws
    lib().ctta_conv_bind_workspace(None, 0)


def _guarded(n, dtype, fill):
    """(whole allocation, the n elements between two guard bands)"""
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _build(c, family, inp, plan):
    """Device buffers of one call.  -> dict(desc, keep, out=(alloc, view), out2=..., gn=...)."""
    nan = float("nan")
    G, B, hs, ws, c0, c1, xs, n, K, M = (c[k] for k in ("groups", "B", "hs", "ws", "c0", "c1", "xs", "n", "K", "M"))
    pix = B * hs * ws
    bx, x = _guarded(pix * xs, torch.bfloat16, nan)
    xv = x.view(pix, xs)
    for g in range(G):
        xv[:, g * c["xgs"]:g * c["xgs"] + c0] = inp["x"][g].reshape(pix, c0).to(torch.bfloat16).to(DEV)
    keep, ptrs = [bx], dict(x0=x.data_ptr())
    if c1:
        b1, x1 = _guarded(pix * c1, torch.bfloat16, nan)
        x1.copy_(inp["x1"].reshape(-1).to(torch.bfloat16))
        keep.append(b1)
        ptrs["x1"] = x1.data_ptr()
    w = torch.full((G, c["n_rows"], c["k_pad"]), nan, dtype=torch.bfloat16, device=DEV)
    w[:, :n] = 0.0
    w[:, :n, :K] = inp["w"].to(torch.bfloat16).to(DEV)
    keep.append(w)
    ptrs["w"] = w.data_ptr()
    if c["bias"]:
        t = inp["bias"].float().to(DEV).contiguous()
        keep.append(t)
        ptrs["bias"] = t.data_ptr()
    if c["bias_m"]:
        t = inp["bias_m"].float().to(DEV).contiguous()
        keep.append(t)
        ptrs["bias_m"] = t.data_ptr()
    if c["rowvec"]:
        t = torch.full((B, n + 4), nan, dtype=torch.float32, device=DEV)
        t[:, :n] = inp["rowvec"].to(DEV)
        keep.append(t)
        ptrs["rowvec"] = t.data_ptr()
    if c["res"]:
        br, r = _guarded(M * (n + 4), torch.bfloat16, nan)
        r.view(M, n + 4)[:, :n] = inp["res"].to(torch.bfloat16).to(DEV)
        keep.append(br)
        ptrs["res"] = r.data_ptr()
    idx = R.dest_index(c)
    odt = torch.float32 if c["out_f32"] else torch.bfloat16
    out = _guarded(R.out_elems(c), odt, R.SENTINEL)
    if c["acc"]:
        out[1][idx[0].reshape(-1).to(DEV)] = inp["old"].reshape(-1).to(odt).to(DEV)
    ptrs["out"] = out[1].data_ptr()
    res = dict(keep=keep, out=out, idx=idx, out2=None, gn=None)
    if c["out2"]:
        res["out2"] = _guarded(R.out_elems(c), torch.bfloat16, R.SENTINEL)
        ptrs["out2"] = res["out2"][1].data_ptr()
    fields = R.desc_fields(c, family)
    if c["gn"]:
        floats = B * plan["gn_nchunk"] * c["gn"] * 2
        res["gn"] = _guarded(floats, torch.float32, R.SENTINEL)
        ptrs["gn_part"] = res["gn"][1].data_ptr()
        fields["gn_part_floats"] = floats
    res["desc"] = R.make_desc(fields, ptrs)
    return res


def _launch(c, dev, workspace):
    L_ = lib()
    if c["ws_bind"]:
        L_.ctta_conv_bind_workspace_ex(N.ptr(workspace), workspace.numel(), 1)
    try:
        N.check(L_.ctta_conv_gemm(ctypes.byref(dev["desc"]), N.stream_ptr()))
        torch.cuda.synchronize()
        return L_.ctta_conv_last_gn_chunks()
    finally:
        if c["ws_bind"]:
            L_.ctta_conv_bind_workspace(None, 0)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                       b.contiguous().view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


def _untouched(c, alloc, idx, what):
    """Everything of an output allocation but the valid elements keeps the sentinel bit for bit."""
    full = alloc.cpu()
    mask = torch.ones(full.numel(), dtype=torch.bool)
    mask[GUARD + idx[idx >= 0].reshape(-1)] = False
    if c["n"] % 4 and c["ldc"] % 4 == 0 and what == "out":          # whole groups of four channels: [n, round_up(n, 4)) hold 0.0
        m = torch.arange(c["M"]).view(-1, 1) * c["ldc"] + torch.arange(c["n"], R.rup(c["n"], 4)).view(1, -1)
        pad = (GUARD + m.reshape(-1))
        assert bool((full[pad].float() == 0.0).all()), "%s: columns [n, round_up(n, 4)) are not 0.0" % c["id"]
        mask[pad] = False
    rest = full[mask]
    assert _same_bits(rest, torch.full_like(rest, R.SENTINEL)), \
        "%s: %d elements of %s outside the valid region were written" % (c["id"], int((rest.float() != R.SENTINEL).sum()), what)


def run_case(c, family, workspace):
    """One launch, every assertion that does not depend on the family.  -> dict(got, got2, ref, routes, plan, ...)"""
    st, pl = R.plan(lib(), c, family)
    assert st == 0, pl
    inp = R.make_inputs(c, family)
    ref = R.reference(c, inp, family)
    dev = _build(c, family, inp, pl)
    chunks = _launch(c, dev, workspace)
    idx = dev["idx"]
    flat = dev["out"][1].cpu()
    valid = idx >= 0
    got = torch.zeros(idx.shape, dtype=torch.float32)
    got[valid] = flat[idx[valid]].float()
    assert bool(torch.isfinite(got).all()), "%s: non-finite output (a poisoned operand was read)" % c["id"]
    if not c["acc"]:
        assert not bool((got[valid] == R.SENTINEL).any()), "%s: a valid element was not written" % c["id"]
    _untouched(c, dev["out"][0], idx, "out")
    got2 = None
    if c["out2"]:
        f2 = dev["out2"][1].cpu()
        got2 = torch.zeros(idx.shape, dtype=torch.float32)
        got2[valid] = f2[idx[valid]].float()
        _untouched(c, dev["out2"][0], idx, "out2")
        s2 = R.slopes(family)["out2_slope"]
        want2 = R.bf16_round(torch.where(got > 0, got, got * s2))
        assert torch.equal(got2[valid], want2[valid]), "%s: out2 is not bf16(leaky(out as stored))" % c["id"]
    geom = R.tile_geom(lib(), pl["variant"]) if pl["variant"] else None
    tgeom = R.tile_geom(lib(), pl["tail_variant"]) if pl["tail_variant"] else None
    routes = R.wave_routes(c, pl, geom, tgeom)
    if c["out_act"] == 4:
        routes = routes[:, R.geglu_cols(c["n"])[0]]
    return dict(got=got, got2=got2, ref=ref, valid=valid, routes=routes, plan=pl, geom=geom, chunks=chunks, dev=dev, inp=inp)


IDS = ["%s-%s" % (c["id"], f) for c, f in R.case_params()]


@pytest.mark.parametrize("case,family", R.case_params(), ids=IDS)
def test_conv_form(case, family, workspace):
    c = case
    r = run_case(c, family, workspace)
    ref, got, valid = r["ref"], r["got"], r["valid"]
    if family in ("integer", "impulse"):
        want, want2 = R.expected_out(c, ref, family)
        bad = (got != want) & valid
        if bool(bad.any()):
            g, m, j = bad.nonzero()[0].tolist()
            pytest.fail("%s/%s: %d elements differ from the exact reference, first at (g, m, n) = (%d, %d, %d): %r stored, %r expected, written by %s"
                        % (c["id"], family, int(bad.sum()), g, m, j, float(got[g, m, j]), float(want[g, m, j]), R.ROUTES[int(r["routes"][m, j])]))
        if c["out2"]:
            assert torch.equal(r["got2"][valid], want2[valid])
        for k in r["routes"].unique().tolist():
            WORST.setdefault((R.ROUTES[k], family), 0.0)
    else:
        err = (got.double() - ref["val"]).abs()
        bnd = R.bound(c, ref, r["plan"])
        ratio = err / bnd.clamp_min(1e-300)
        fails = []
        for k in r["routes"].unique().tolist():
            sel = (r["routes"] == k).unsqueeze(0) & valid
            w = R.worst_ratio(err[sel], bnd[sel])
            key = (R.ROUTES[k], family)
            WORST[key] = max(WORST.get(key, 0.0), w)
            print("%s/%s %s: worst error / bound %.3f, worst error %.3e, over %d elements" % (c["id"], family, R.ROUTES[k], w, float(err[sel].max()), int(sel.sum())))
            if not w < 1.0:
                fails.append((R.ROUTES[k], w, int((ratio[sel] >= 1.0).sum())))
        assert not fails, "%s/%s: (route, worst error / bound, elements over the bound) %r" % (c["id"], family, fails)
    if c["gn"]:
        pl, geom = r["plan"], r["geom"]
        assert r["chunks"] == pl["gn_nchunk"] > 0
        part = r["dev"]["gn"][1].cpu().double().view(c["B"], pl["gn_nchunk"], c["gn"], 2)
        _untouched(c, r["dev"]["gn"][0], torch.arange(part.numel()), "gn_part")
        want, _, _ = R.gn_reference(c, ref, pl, geom)
        gb = R.gn_bound(c, ref, pl, geom)
        w = R.worst_ratio((part - want).abs(), gb)
        # which partials hold elements of waves on the generic epilogue (column-edge waves; every wave behind an activation)
        edge = (r["routes"] != R.ROUTES.index("fast")).any(0).view(c["gn"], -1).any(1)
        for name, sel in (("gn:fast", ~edge), ("gn:wide4", edge)):
            if bool(sel.any()):
                ws_ = R.worst_ratio((part - want).abs()[:, :, sel], gb[:, :, sel])
                WORST[(name, family)] = max(WORST.get((name, family), 0.0), ws_)
                print("%s/%s %s: worst partial error / bound %.3f" % (c["id"], family, name, ws_))
        assert w < 1.0, "%s/%s: GroupNorm partials, worst error / bound %.3f" % (c["id"], family, w)
        if family == "integer":          # integers + 1/64: the sums of the unrounded values are exact in fp32 in any order
            bad = part[..., 0] != want[..., 0]
            assert not bool(bad.any()), "%s: %d of %d GroupNorm sums are not the sums of the unrounded values, first (sample, chunk, group) %s: %r vs %r" % (
                c["id"], int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()), float(part[..., 0][bad][0]), float(want[..., 0][bad][0]))
    else:
        assert r["chunks"] == 0


@pytest.mark.parametrize("sfx", ["c40", "cat"])
@pytest.mark.parametrize("i", range(1, 9))
def test_staging_modes_0_and_1_give_the_same_bits(i, sfx, workspace):
    """Tiles i and i + 8 are the same tile with register staging and with the generic direct-to-LDS gather: one K walk (channels
    innermost, a K tile may straddle taps and the source boundary), one MFMA order, one epilogue -- the same bits.  (The MODE 2
    twin i + 16 walks K with the taps innermost and is held to the bound and to the integer family only.)"""
    outs = []
    for t in (i, i + 8):
        c = R.BY_ID["t%d-%s" % (t, sfx)]
        _, pl = R.plan(lib(), c)
        dev = _build(c, "uniform", R.make_inputs(R.BY_ID["t%d-%s" % (i, sfx)], "uniform"), pl)          # the same inputs for both
        _launch(c, dev, workspace)
        outs.append(dev["out"][0].cpu())
    assert _same_bits(outs[0], outs[1])


@pytest.mark.parametrize("tile", R.EPI_TILES)
def test_an_element_has_the_same_bits_on_the_straight_line_and_on_the_generic_route(tile, workspace):
    """"Every epilogue of the library adds in this order -- acc + (bias + rowvec), then the residual, then the old output -- so
    that a sample's numbers do not depend on which path its tile took" (wide_epilogue_fast).  One 1x1 problem launched twice on
    the same tile: as two samples of 1.5 BM rows (the middle row tile straddles them: generic epilogue_wide4) and as ONE sample
    of 3 BM rows (every full wave straight-line), with the same row vector for both samples.  The K walk is the same launch
    for launch, so the outputs differ exactly when the two epilogue codes do.  The inputs make a reordering visible in the
    stored bf16 bits: res = +4096 and old out = -4096 cancel, so the sum in front of them is rounded to 2^-11 on the way."""
    g = R.tile_geom(lib(), tile)
    hw = g["bm"] + g["bm"] // 2
    kw = dict(c0=64, n=72, tile=tile, bias=1, rowvec=1, res=1, acc=1, ws=1)
    two, one = R._case("inv-two", [], B=2, hs=hw, **kw), R._case("inv-one", [], B=1, hs=2 * hw, **kw)
    inp = R.make_inputs(two, "uniform")
    inp["rowvec"][1] = inp["rowvec"][0]
    inp["res"], inp["old"] = torch.full_like(inp["res"], 4096.0), torch.full_like(inp["old"], -4096.0)
    outs, routes = [], []
    for c, i in ((two, inp), (one, dict(inp, rowvec=inp["rowvec"][:1], x=inp["x"].reshape(1, 1, 2 * hw, 1, 64)))):
        st, pl = R.plan(lib(), c)
        assert st == 0 and pl["variant"] == tile and pl["epi_fast"] == 1
        dev = _build(c, "uniform", i, pl)
        _launch(c, dev, workspace)
        outs.append(dev["out"][0].cpu())
        routes.append(R.wave_routes(c, pl, g))
    moved = (routes[0] == R.ROUTES.index("wide4_sample")) & (routes[1] == R.ROUTES.index("fast"))
    assert int(moved.sum()) >= g["bm"] * 64          # a whole row tile x the full waves' columns changes its code
    assert bool(torch.isfinite(outs[0].float()).all()) and float(outs[0][GUARD:GUARD + 72].float().abs().max()) < 64
    assert _same_bits(outs[0], outs[1])


@pytest.mark.parametrize("case", [c for c in R.CASES if c.get("refused")], ids=[c["id"] for c in R.CASES if c.get("refused")])
def test_refused_forms_are_errors(case, workspace):
    st, err = R.plan(lib(), case)
    assert st != 0 and case["refused"] in err
    inp = R.make_inputs(case, case["families"][0])
    dev = _build(case, case["families"][0], inp, dict(gn_nchunk=0))
    with pytest.raises(N.CttaError):
        _launch(case, dev, workspace)
    assert case["refused"] in lib().ctta_last_error().decode()
    assert _same_bits(dev["out"][0].cpu(), torch.full_like(dev["out"][0].cpu(), R.SENTINEL))


def test_report():
    """Worst error / bound per epilogue code and input family over the cases that ran (LABNOTES.md quotes it).  Always passes."""
    for (route, fam), w in sorted(WORST.items()):
        print("conv_forms worst error/bound  %-14s %-8s %.3f" % (route, fam, w))
