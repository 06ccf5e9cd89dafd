"""The fused LoRA site kernels (csrc/lora.hip: ctta_lora_sites_fwd / _bwd) against the per-site launches they replace.

Layouts and conventions are those of tests/test_lora_ops_gpu.py: a logical width in a padded one, zeros in the packed
adapter's padding, 1e30 in the activations' padded columns, the [q | k] buffer addressed by offset.  What is compared:
  forward   D and every Y bit for bit with ctta_lora_down(a_kmajor=0) + ctta_lora_up_add(b_rmajor=0) / ctta_lora_up_add_t
  backward  dD bit for bit with ctta_lora_down(a_kmajor=1); dX bit for bit with one ctta_lora_up_add(b_rmajor=1) per site in
            site order; gA / gB against float64 within M u sum|terms| (the bound test_lora_ops_gpu.py states for wgrad) at
            scale 1; two runs bit-identical; into a non-zero G at 1..3 floats off a 16-byte boundary exactly fl(G + value);
            columns the map sends to -1 untouched
"""
import pytest
import torch

from consistencytta_amd import _native as N
from gpu_util import DEV, bf16_round, det, sync
from test_lora_ops_gpu import BIG, LAYOUTS as BASE_LAYOUTS, U, ident, packed, padded_act

pytestmark = pytest.mark.gpu

MS = (1, 63, 65, 257, 1031)
RANKS = (1, 2, 4)
LAYOUTS = {k: BASE_LAYOUTS[k] for k in ("39in64", "255in256", "320", "3x13in192")}
LAYOUTS["1024"] = ident(1024, 1024)
LAYOUTS["1280"] = ident(1280, 1280)
WIDE = ("1024", "1280")
# the output layout of a site whose input has layout `lay`: the same, except that the text width projects to an inner width
OUT_OF = {"1024": "255in256"}


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


BIG_M = 36872      # slabs of 80 rows: more than one 64-row tile per slab, as at the engines' 36864 rows


def ms_of(lay):
    if lay in WIDE:
        return (65,)
    return MS + (BIG_M,) if lay == "255in256" else MS


def skip_combo(m, r, ns):
    """the large row count runs once: rank 4, three sites"""
    return m == BIG_M and (r != 4 or ns != 3)


def adapters(lay, r, ns, zero_up=False):
    """per site: logical a (r, k), b (n, r), and their packed forms [r][k_pad] / [n_pad][r]"""
    lin, lout = LAYOUTS[lay], LAYOUTS[OUT_OF.get(lay, lay)]
    out = []
    for s in range(ns):
        al = det("sites.a.%s.%d.%d" % (lay, r, s), (r, lin[0]), scale=0.5)
        bl = det("sites.b.%s.%d.%d" % (lay, r, s), (lout[0], r), scale=0.5)
        if zero_up:
            bl = torch.zeros_like(bl)
        out.append((al, bl, packed(al, lin, 1), packed(bl, lout, 0)))
    return lin, lout, out


def dest_buffers(name, m, lout, ns):
    """destinations of `ns` sites: one plain site; a [q | k] pair in one buffer of twice the width; the pair + a plain site.
    -> [(buffer, ld, column offset)], buffers shared where two sites live in one"""
    pad = lout[1]
    if ns == 1:
        return [(padded_act(name + ".0", m, lout, pad, 0)[1], pad, 0)]
    yl0, qk = padded_act(name + ".q", m, lout, 2 * pad, 0)
    qk[:, pad + lout[2]] = bf16_round(det(name + ".k", (m, lout[0]))).to(torch.bfloat16).to(DEV)
    dst = [(qk, 2 * pad, 0), (qk, 2 * pad, pad)]
    if ns == 3:
        dst.append((padded_act(name + ".2", m, lout, pad, 0)[1], pad, 0))
    return dst


def clone_dests(dst):
    seen = {}
    out = []
    for buf, ld, off in dst:
        if id(buf) not in seen:
            seen[id(buf)] = buf.clone()
        out.append((seen[id(buf)], ld, off))
    return out


def fwd_sites(ad, dst, ds, vt=None):
    arr = (N.LoraFwdSite * len(ad))()
    for s, ((al, bl, a, b), (buf, ld, off)) in enumerate(zip(ad, dst)):
        arr[s].a, arr[s].b, arr[s].d = N.ptr(a), N.ptr(b), N.ptr(ds[s])
        arr[s].n_pad = b.shape[0]
        if vt is not None and s == len(ad) - 1:
            tokens, ldt = vt
            arr[s].y, arr[s].ldy, arr[s].tokens, arr[s].batch_stride = N.ptr(buf), ldt, tokens, b.shape[0] * ldt
        else:
            arr[s].y, arr[s].ldy, arr[s].tokens, arr[s].batch_stride = N.ptr(buf[:, off:]), ld, 0, 0
    return arr


@pytest.mark.parametrize("lay", sorted(LAYOUTS))
def test_forward_is_bit_for_bit_the_two_launch_route(lay):
    L = N.lib()
    for m in ms_of(lay):
        for r in RANKS:
            for ns in (1, 2, 3):
                if skip_combo(m, r, ns):
                    continue
                lin, lout, ad = adapters(lay, r, ns)
                xl, x = padded_act("sites.fx.%s.%d" % (lay, m), m, lin, lin[1], 0)
                dst0 = dest_buffers("sites.fy.%s.%d" % (lay, m), m, lout, ns)
                for scale in (1.0, 0.75):
                    ref, got = clone_dests(dst0), clone_dests(dst0)
                    d_ref = [torch.full((m, r), float("nan"), device=DEV) for _ in range(ns)]
                    d_got = [torch.full((m, r), float("nan"), device=DEV) for _ in range(ns)]
                    for s, ((al, bl, a, b), (buf, ld, off)) in enumerate(zip(ad, ref)):
                        N.check(L.ctta_lora_down(N.ptr(x), lin[1], m, lin[1], N.ptr(a), 0, r, N.ptr(d_ref[s]), N.stream_ptr()))
                        N.check(L.ctta_lora_up_add(N.ptr(buf[:, off:]), ld, m, lout[1], N.ptr(d_ref[s]), N.ptr(b), 0, r, scale,
                                                   N.stream_ptr()))
                    N.check(L.ctta_lora_sites_fwd(N.ptr(x), lin[1], m, lin[1], r, scale, fwd_sites(ad, got, d_got), ns,
                                                  N.stream_ptr()))
                    sync()
                    for s in range(ns):
                        assert same_bits(d_got[s], d_ref[s]), ("D", lay, m, r, ns, s, scale)
                        assert same_bits(got[s][0], ref[s][0]), ("Y", lay, m, r, ns, s, scale)
                        # the route was not a no-op, and nothing outside the logical columns moved
                        buf, ld, off = got[s]
                        keep = torch.ones(ld, dtype=torch.bool)
                        for t in range(ns):
                            if got[t][0] is buf:
                                keep[got[t][2] + lout[2]] = False
                        assert same_bits(buf[:, keep], dst0[s][0][:, keep])
                        assert not same_bits(buf, dst0[s][0])
                # zero `up`: Y bit for bit, D still written
                _, _, adz = adapters(lay, r, ns, zero_up=True)
                got = clone_dests(dst0)
                d_got = [torch.full((m, r), float("nan"), device=DEV) for _ in range(ns)]
                N.check(L.ctta_lora_sites_fwd(N.ptr(x), lin[1], m, lin[1], r, 1.0, fwd_sites(adz, got, d_got), ns, N.stream_ptr()))
                sync()
                for s in range(ns):
                    assert same_bits(got[s][0], dst0[s][0]) and bool(torch.isfinite(d_got[s]).all())


@pytest.mark.parametrize("batch,tokens,ldt", [(3, 24, 24), (2, 72, 80), (1, 1032, 1032), (11, 3352, 3352)])
def test_forward_into_a_transposed_destination(batch, tokens, ldt):
    """a [q | k] pair plus V^T [batch][n_pad][ldt] with 8 | tokens (and alone, as the cross-attention's k / v group has it)"""
    L = N.lib()
    m = batch * tokens
    for lay in ("3x13in192", "255in256"):
        for r in RANKS:
            for ns in (1, 3):
                if m == BIG_M and (lay != "3x13in192" or skip_combo(m, r, ns)):
                    continue
                lin, lout, ad = adapters(lay, r, ns)
                n, pad, pos = lout
                xl, x = padded_act("sites.tx.%s.%d" % (lay, m), m, lin, lin[1], 0)
                dst0 = dest_buffers("sites.ty.%s.%d" % (lay, m), m, lout, ns - 1) if ns > 1 else []
                yt0 = torch.full((batch, pad, ldt), BIG)
                yt0[:, pos, :tokens] = bf16_round(det("sites.tyt.%s.%d" % (lay, m), (batch, n, tokens)))
                yt0 = yt0.to(torch.bfloat16).to(DEV)
                dst0 = dst0 + [(yt0, ldt, 0)]
                for scale in (1.0, 0.75):
                    ref, got = clone_dests(dst0), clone_dests(dst0)
                    d_ref = [torch.full((m, r), float("nan"), device=DEV) for _ in range(ns)]
                    d_got = [torch.full((m, r), float("nan"), device=DEV) for _ in range(ns)]
                    for s, ((al, bl, a, b), (buf, ld, off)) in enumerate(zip(ad, ref)):
                        N.check(L.ctta_lora_down(N.ptr(x), lin[1], m, lin[1], N.ptr(a), 0, r, N.ptr(d_ref[s]), N.stream_ptr()))
                        if s == ns - 1:
                            N.check(L.ctta_lora_up_add_t(N.ptr(buf), ldt, pad * ldt, batch, tokens, pad, N.ptr(d_ref[s]), tokens,
                                                         N.ptr(b), r, scale, N.stream_ptr()))
                        else:
                            N.check(L.ctta_lora_up_add(N.ptr(buf[:, off:]), ld, m, pad, N.ptr(d_ref[s]), N.ptr(b), 0, r, scale,
                                                       N.stream_ptr()))
                    N.check(L.ctta_lora_sites_fwd(N.ptr(x), lin[1], m, lin[1], r, scale,
                                                  fwd_sites(ad, got, d_got, vt=(tokens, ldt)), ns, N.stream_ptr()))
                    sync()
                    for s in range(ns):
                        assert same_bits(d_got[s], d_ref[s]), ("D", lay, m, r, ns, s, scale)
                        assert same_bits(got[s][0], ref[s][0]), ("Y", lay, m, r, ns, s, scale)
                    assert not same_bits(got[-1][0], yt0)
                    keep = torch.ones(pad, ldt, dtype=torch.bool)
                    keep[pos, :tokens] = False
                    assert same_bits(got[-1][0][:, keep], yt0[:, keep])
                _, _, adz = adapters(lay, r, ns, zero_up=True)
                got = clone_dests(dst0)
                d_got = [torch.full((m, r), float("nan"), device=DEV) for _ in range(ns)]
                N.check(L.ctta_lora_sites_fwd(N.ptr(x), lin[1], m, lin[1], r, 1.0, fwd_sites(adz, got, d_got, vt=(tokens, ldt)),
                                              ns, N.stream_ptr()))
                sync()
                assert all(same_bits(got[s][0], dst0[s][0]) for s in range(ns))


def bwd_sites(ad, dys, ds, dds, gas, gbs, kmap, nmap, k, r):
    arr = (N.LoraBwdSite * len(ad))()
    for s, ((al, bl, a, b), (buf, ld, off)) in enumerate(zip(ad, dys)):
        arr[s].dy, arr[s].lddy, arr[s].n_pad = N.ptr(buf[:, off:]), ld, b.shape[0]
        arr[s].a, arr[s].b, arr[s].d, arr[s].dd = N.ptr(a), N.ptr(b), N.ptr(ds[s]), N.ptr(dds[s])
        if gas is not None:
            arr[s].ga, arr[s].gb, arr[s].k_map, arr[s].n_map = N.ptr(gas[s]), N.ptr(gbs[s]), N.ptr(kmap), N.ptr(nmap)
            arr[s].ga_stride_r, arr[s].ga_stride_k, arr[s].gb_stride_r, arr[s].gb_stride_k = k, 1, 1, r
    return arr


def col_map_of(layout, drop=None):
    n, pad, pos = layout
    cm = torch.full((pad,), -1, dtype=torch.int32)
    cm[pos] = torch.arange(n, dtype=torch.int32)
    if drop is not None:
        cm[pos[drop]] = -1
    return cm.to(DEV)


@pytest.mark.parametrize("lay", sorted(LAYOUTS))
def test_backward(lay):
    L = N.lib()
    for m in ms_of(lay):
        for r in RANKS:
            for ns in (1, 2, 3):
                if skip_combo(m, r, ns):
                    continue
                lin, lout, ad = adapters(lay, r, ns)
                k, kpad, kpos = lin
                n, npad, npos = lout
                xl, x = padded_act("sites.bx.%s.%d" % (lay, m), m, lin, kpad, 0)
                dys = dest_buffers("sites.bdy.%s.%d" % (lay, m), m, lout, ns)          # dq | dk in one buffer, dv plain
                dyl = [dys[s][0].float().cpu()[:, dys[s][2] + npos].double() for s in range(ns)]
                _, dx0 = padded_act("sites.bdx.%s.%d" % (lay, m), m, lin, kpad, 0)
                ds = [det("sites.bd.%s.%d.%d.%d" % (lay, m, r, s), (m, r)).to(DEV) for s in range(ns)]
                kmap, nmap = col_map_of(lin), col_map_of(lout)
                nf = L.ctta_lora_sites_bwd_scratch_floats(m, kpad, npad, ns, r)
                assert nf > 0
                scratch = torch.empty(nf, device=DEV)

                def run(dx, gas, gbs, scale, dds, km=kmap, nm=nmap):
                    N.check(L.ctta_lora_sites_bwd(N.ptr(x), kpad, N.ptr(dx), kpad, m, kpad, r, scale,
                                                  bwd_sites(ad, dys, ds, dds, gas, gbs, km, nm, k, r), ns, N.ptr(scratch),
                                                  N.stream_ptr()))
                    sync()

                for scale in (1.0, 0.75):
                    # the per-site route: dD, then dX site by site
                    dd_ref = [torch.full((m, r), float("nan"), device=DEV) for _ in range(ns)]
                    dx_ref = dx0.clone()
                    for s, ((al, bl, a, b), (buf, ld, off)) in enumerate(zip(ad, dys)):
                        N.check(L.ctta_lora_down(N.ptr(buf[:, off:]), ld, m, npad, N.ptr(b), 1, r, N.ptr(dd_ref[s]), N.stream_ptr()))
                        N.check(L.ctta_lora_up_add(N.ptr(dx_ref), kpad, m, kpad, N.ptr(dd_ref[s]), N.ptr(a), 1, r, scale,
                                                   N.stream_ptr()))
                    dd = [torch.full((m, r), float("nan"), device=DEV) for _ in range(ns)]
                    dx = dx0.clone()
                    ga = [torch.zeros(r, k, device=DEV) for _ in range(ns)]
                    gb = [torch.zeros(n, r, device=DEV) for _ in range(ns)]
                    run(dx, ga, gb, scale, dd)
                    for s in range(ns):
                        assert same_bits(dd[s], dd_ref[s]), ("dD", lay, m, r, ns, s)
                    assert same_bits(dx, dx_ref), ("dX", lay, m, r, ns, scale)
                    assert not same_bits(dx, dx0)
                    if scale == 1.0:   # the float64 bound, on the inputs the kernels saw (dD as they formed it)
                        for s in range(ns):
                            d64, dd64 = ds[s].cpu().double(), dd[s].cpu().double()
                            ref_b, abs_b = dyl[s].t() @ d64, dyl[s].abs().t() @ d64.abs()              # (n, r)
                            ref_a, abs_a = dd64.t() @ xl.double(), dd64.abs().t() @ xl.double().abs()  # (r, k)
                            eb = (gb[s].cpu().double() - ref_b).abs()
                            ea = (ga[s].cpu().double() - ref_a).abs()
                            assert bool((eb <= m * U * abs_b + 1e-30).all()), ("gB", lay, m, r, ns, s, float((eb / (m * U * abs_b + 1e-30)).max()))
                            assert bool((ea <= m * U * abs_a + 1e-30).all()), ("gA", lay, m, r, ns, s, float((ea / (m * U * abs_a + 1e-30)).max()))
                    # two runs give the same bits
                    ga2 = [torch.zeros(r, k, device=DEV) for _ in range(ns)]
                    gb2 = [torch.zeros(n, r, device=DEV) for _ in range(ns)]
                    dx2 = dx0.clone()
                    run(dx2, ga2, gb2, scale, dd)
                    assert same_bits(dx2, dx) and all(same_bits(ga2[s], ga[s]) and same_bits(gb2[s], gb[s]) for s in range(ns))
                    # no parameter gradients wanted: the same dD and dX
                    dx3 = dx0.clone()
                    dd3 = [torch.full((m, r), float("nan"), device=DEV) for _ in range(ns)]
                    run(dx3, None, None, scale, dd3)
                    assert same_bits(dx3, dx) and all(same_bits(dd3[s], dd[s]) for s in range(ns))
                # scale 0.5 into a non-zero G at every fp32 alignment: exactly fl(G + value); dropped columns keep their bits
                za = [torch.zeros(r, k, device=DEV) for _ in range(ns)]
                zb = [torch.zeros(n, r, device=DEV) for _ in range(ns)]
                run(dx0.clone(), za, zb, 0.5, dd)
                drop_k, drop_n = torch.arange(0, k, 3), torch.arange(1, n, 3)
                km, nm = col_map_of(lin, drop_k), col_map_of(lout, drop_n)
                for shift in (0, 1, 2, 3):
                    bufa = [torch.zeros(r * k + 8, device=DEV) for _ in range(ns)]
                    bufb = [torch.zeros(n * r + 8, device=DEV) for _ in range(ns)]
                    g0a = det("sites.g0a.%s.%d" % (lay, r), (r, k)).to(DEV)
                    g0b = det("sites.g0b.%s.%d" % (lay, r), (n, r)).to(DEV)
                    ga = [b_[shift:shift + r * k].view(r, k) for b_ in bufa]
                    gb = [b_[shift:shift + n * r].view(n, r) for b_ in bufb]
                    for s in range(ns):
                        ga[s].copy_(g0a)
                        gb[s].copy_(g0b)
                        assert ga[s].data_ptr() % 16 == 4 * shift
                    run(dx0.clone(), ga, gb, 0.5, dd, km, nm)
                    for s in range(ns):
                        wa, wb = g0a + za[s], g0b + zb[s]
                        wa[:, drop_k] = g0a[:, drop_k]
                        wb[drop_n, :] = g0b[drop_n, :]
                        assert same_bits(ga[s], wa) and same_bits(gb[s], wb), (lay, m, r, ns, s, shift)
                        for b_, cnt in ((bufa[s], r * k), (bufb[s], n * r)):
                            assert float(b_[:shift].abs().sum()) == 0 and float(b_[shift + cnt:].abs().sum()) == 0


def test_backward_without_an_input_gradient():
    """the text states: dx NULL, two sites, parameter gradients only"""
    L = N.lib()
    lay, m, r, ns = "1024", 65, 4, 2
    lin, lout, ad = adapters(lay, r, ns)
    k, kpad, kpos = lin
    n, npad, npos = lout
    xl, x = padded_act("sites.nx", m, lin, kpad, 0)
    dys = [(padded_act("sites.ndy.%d" % s, m, lout, npad, 0)[1], npad, 0) for s in range(ns)]
    ds = [det("sites.nd.%d" % s, (m, r)).to(DEV) for s in range(ns)]
    dd = [torch.full((m, r), float("nan"), device=DEV) for _ in range(ns)]
    ga = [torch.zeros(r, k, device=DEV) for _ in range(ns)]
    gb = [torch.zeros(n, r, device=DEV) for _ in range(ns)]
    scratch = torch.empty(L.ctta_lora_sites_bwd_scratch_floats(m, kpad, npad, ns, r), device=DEV)
    N.check(L.ctta_lora_sites_bwd(N.ptr(x), kpad, None, 0, m, kpad, r, 1.0,
                                  bwd_sites(ad, dys, ds, dd, ga, gb, col_map_of(lin), col_map_of(lout), k, r), ns, N.ptr(scratch),
                                  N.stream_ptr()))
    sync()
    for s in range(ns):
        ref = torch.full((m, r), float("nan"), device=DEV)
        N.check(L.ctta_lora_down(N.ptr(dys[s][0]), npad, m, npad, N.ptr(ad[s][3]), 1, r, N.ptr(ref), N.stream_ptr()))
        sync()
        assert same_bits(dd[s], ref)
        dd64 = dd[s].cpu().double()
        ea = (ga[s].cpu().double() - dd64.t() @ xl.double()).abs()
        assert bool((ea <= m * U * (dd64.abs().t() @ xl.double().abs()) + 1e-30).all())
        dyl = dys[s][0].float().cpu()[:, npos].double()
        eb = (gb[s].cpu().double() - dyl.t() @ ds[s].cpu().double()).abs()
        assert bool((eb <= m * U * (dyl.abs().t() @ ds[s].cpu().double().abs()) + 1e-30).all())


def test_bad_arguments_are_refused():
    L = N.lib()
    t = torch.zeros(64, 64, dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(64 * 64, device=DEV)
    site = (N.LoraFwdSite * 1)()
    site[0].a, site[0].b, site[0].y, site[0].ldy, site[0].n_pad = N.ptr(f), N.ptr(f), N.ptr(t), 64, 64
    assert L.ctta_lora_sites_fwd(N.ptr(t), 64, 4, 64, 5, 1.0, site, 1, N.stream_ptr()) != 0        # rank
    assert L.ctta_lora_sites_fwd(N.ptr(t), 64, 4, 64, 4, 1.0, site, 4, N.stream_ptr()) != 0        # sites
    assert L.ctta_lora_sites_fwd(N.ptr(t), 32, 4, 64, 4, 1.0, site, 1, N.stream_ptr()) != 0        # ld < k
    site[0].tokens, site[0].batch_stride = 4, 64 * 64                                              # 4 tokens: not the vector path
    assert L.ctta_lora_sites_fwd(N.ptr(t), 64, 4, 64, 4, 1.0, site, 1, N.stream_ptr()) != 0
