"""The LoRA adapter kernels (csrc/lora.hip) one by one against float64 torch on the same bf16-rounded inputs.

Layouts are the engines': a logical width sits in a padded one (identity padding to a multiple of 64, or heads of dh
lanes in 64-wide head blocks), the packed adapter holds zeros in every padded row / column, and the activations' padded
columns are filled with a large finite value here (the engines write zeros there): the results must not depend on them.

Bounds (fp32 accumulation, u = 2^-24; one bf16 rounding = 2^-9 relative, asserted as 2^-8):
  down    |got - ref| <= K u sum|x a|
  up_add  |got - ref| <= 2^-8 |ref| + r u sum|terms|, and zero adapters leave Y bit for bit
  wgrad   |got - ref| <= M u sum|terms| into a zeroed G; into a non-zero G the result is exactly fl(G + that), at any
          fp32 address (1..3 floats off a 16-byte boundary); two runs are bit-identical
"""
import pytest
import torch

from consistencytta_amd import _native as N
from gpu_util import DEV, bf16_round, det, sync

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BIG = 1.0e30          # finite in bf16; what a padded activation column holds in these tests
MS = (1, 63, 65, 257)
RANKS = (1, 4, 16)


def ident(n, pad):
    return n, pad, torch.arange(n)


def heads(h, dh):
    return h * dh, h * 64, torch.cat([torch.arange(dh) + 64 * i for i in range(h)])


# logical width, padded width, padded position of every logical column
LAYOUTS = {"39in64": ident(39, 64), "63in64": ident(63, 64), "255in256": ident(255, 256), "320": ident(320, 320),
           "3x13in192": heads(3, 13)}


def padded_act(name, m, layout, ld, off, fill=BIG):
    """logical (m, n) bf16-rounded values, and a (m, ld) bf16 device matrix that holds them at `off` + their padded
    positions, `fill` everywhere else"""
    n, pad, pos = layout
    xl = bf16_round(det(name, (m, n)))
    x = torch.full((m, ld), fill, dtype=torch.float32)
    x[:, off + pos] = xl
    return xl, x.to(torch.bfloat16).to(DEV)


def packed(wl, layout, axis):
    """logical matrix -> zeros-padded along `axis` (fp32, device)"""
    n, pad, pos = layout
    shape = list(wl.shape)
    shape[axis] = pad
    w = torch.zeros(shape)
    w.index_copy_(axis, pos, wl)
    return w.contiguous().to(DEV)


def buffers(pad):
    """leading dimensions to run at: the width itself, and a [q | k] buffer of twice the width with the second half
    addressed by offset"""
    return ((pad, 0), (2 * pad, pad))


@pytest.mark.parametrize("lay", sorted(LAYOUTS))
def test_down(lay):
    L = N.lib()
    layout = LAYOUTS[lay]
    k, pad, pos = layout
    for m in MS:
        for r in RANKS:
            al = det("lora.down.a.%s.%d" % (lay, r), (r, k), scale=0.5)
            a_rk = packed(al, layout, 1)                 # [r][k_pad]
            a_kr = a_rk.t().contiguous()                 # [k_pad][r]
            for ld, off in buffers(pad):
                xl, x = padded_act("lora.down.x.%s.%d" % (lay, m), m, layout, ld, off)
                ref = xl.double() @ al.double().t()
                bound = k * U * (xl.double().abs() @ al.double().abs().t()) + 1e-30
                for kmajor, a in ((0, a_rk), (1, a_kr)):
                    d = torch.full((m, r), float("nan"), device=DEV)
                    N.check(L.ctta_lora_down(N.ptr(x[:, off:]), ld, m, pad, N.ptr(a), kmajor, r, N.ptr(d), N.stream_ptr()))
                    sync()
                    err = (d.cpu().double() - ref).abs()
                    assert bool((err <= bound).all()), (lay, m, r, ld, kmajor, float((err / bound).max()))


@pytest.mark.parametrize("lay", sorted(LAYOUTS))
def test_up_add(lay):
    L = N.lib()
    layout = LAYOUTS[lay]
    n, pad, pos = layout
    for m in MS:
        for r in RANKS:
            bl = det("lora.up.b.%s.%d" % (lay, r), (n, r), scale=0.5)
            b_nr = packed(bl, layout, 0)                 # [n_pad][r]
            b_rn = b_nr.t().contiguous()                 # [r][n_pad]
            dd = det("lora.up.d.%s.%d.%d" % (lay, m, r), (m, r))
            dd_dev, b_zero = dd.to(DEV), torch.zeros_like(b_nr)
            for ld, off in buffers(pad):
                yl, y0 = padded_act("lora.up.y.%s.%d" % (lay, m), m, layout, ld, off)
                for scale in (1.0, 0.75):
                    terms = scale * dd.double()[:, None, :] * bl.double()[None, :, :]            # (m, n, r)
                    ref = yl.double() + terms.sum(-1)
                    bound = 2.0 ** -8 * ref.abs() + r * U * terms.abs().sum(-1) + 1e-30
                    for rmajor, b in ((0, b_nr), (1, b_rn)):
                        y = y0.clone()
                        N.check(L.ctta_lora_up_add(N.ptr(y[:, off:]), ld, m, pad, N.ptr(dd_dev), N.ptr(b), rmajor, r, scale,
                                                   N.stream_ptr()))
                        sync()
                        got = y.float().cpu()
                        err = (got[:, off + pos].double() - ref).abs()
                        assert bool((err <= bound).all()), (lay, m, r, ld, rmajor, float((err / bound).max()))
                        # everything else (padded columns, the other half of a [q | k] buffer) keeps its bits
                        keep = torch.ones(ld, dtype=torch.bool)
                        keep[off + pos] = False
                        assert torch.equal(y.view(torch.int16).cpu()[:, keep], y0.view(torch.int16).cpu()[:, keep])
                # zero adapters: Y unchanged
                y = y0.clone()
                N.check(L.ctta_lora_up_add(N.ptr(y[:, off:]), ld, m, pad, N.ptr(dd_dev), N.ptr(b_zero), 0, r, 1.0,
                                           N.stream_ptr()))
                sync()
                assert torch.equal(y, y0) and torch.equal(y.view(torch.int16), y0.view(torch.int16))


@pytest.mark.parametrize("tokens,ldt", [(4, 8), (13, 16), (64, 64), (6 * 8, 48)])
def test_up_add_transposed(tokens, ldt):
    """V^T [batch][n_pad][ldt]: the 8-token vector path (tokens a multiple of 8) and the scalar one"""
    L = N.lib()
    layout = LAYOUTS["3x13in192"]
    n, pad, pos = layout
    batch = 3
    for r in RANKS:
        bl = det("lora.upt.b.%d" % r, (n, r), scale=0.5)
        b = packed(bl, layout, 0)
        dd = det("lora.upt.d.%d.%d" % (tokens, r), (batch * tokens, r))
        dd_dev, b_zero = dd.to(DEV), torch.zeros_like(b)
        yl = bf16_round(det("lora.upt.y.%d" % tokens, (batch, n, tokens)))
        y0 = torch.full((batch, pad, ldt), BIG)
        y0[:, pos, :tokens] = yl
        y0 = y0.to(torch.bfloat16).to(DEV)
        y = y0.clone()
        N.check(L.ctta_lora_up_add_t(N.ptr(y), ldt, pad * ldt, batch, tokens, pad, N.ptr(dd_dev), tokens, N.ptr(b), r, 1.0,
                                     N.stream_ptr()))
        sync()
        terms = dd.double().reshape(batch, 1, tokens, r) * bl.double().reshape(1, n, 1, r)
        ref = yl.double() + terms.sum(-1)
        bound = 2.0 ** -8 * ref.abs() + r * U * terms.abs().sum(-1) + 1e-30
        got = y.float().cpu()
        err = (got[:, pos, :tokens].double() - ref).abs()
        assert bool((err <= bound).all()), (tokens, r, float((err / bound).max()))
        keep = torch.ones(pad, ldt, dtype=torch.bool)
        keep[pos, :tokens] = False
        assert torch.equal(y.view(torch.int16).cpu()[:, keep], y0.view(torch.int16).cpu()[:, keep])
        z = y0.clone()
        N.check(L.ctta_lora_up_add_t(N.ptr(z), ldt, pad * ldt, batch, tokens, pad, N.ptr(dd_dev), tokens, N.ptr(b_zero), r, 1.0,
                                     N.stream_ptr()))
        sync()
        assert torch.equal(z.view(torch.int16), y0.view(torch.int16))


@pytest.mark.parametrize("lay", sorted(LAYOUTS))
def test_wgrad(lay):
    L = N.lib()
    layout = LAYOUTS[lay]
    k, pad, pos = layout
    col_map = torch.full((pad,), -1, dtype=torch.int32)
    col_map[pos] = torch.arange(k, dtype=torch.int32)
    col_map = col_map.to(DEV)
    for m in MS + (4100,):                                       # 4100 rows: 17 partial slabs are folded
        for r in RANKS if m != 4100 else (4,):
            dd = det("lora.wg.d.%s.%d.%d" % (lay, m, r), (m, r))
            dd_dev = dd.to(DEV)
            nf = L.ctta_lora_wgrad_scratch_floats(m, pad, r)
            assert nf >= r * pad and (m != 4100 or nf == 17 * r * pad)
            scratch = torch.empty(nf, device=DEV)
            for ld, off in buffers(pad):
                xl, x = padded_act("lora.wg.x.%s.%d" % (lay, m), m, layout, ld, off)
                terms_abs = dd.double().abs().t() @ xl.double().abs()                       # (r, k)
                ref = dd.double().t() @ xl.double()

                def run(g, sr, sk, scale=1.0):
                    N.check(L.ctta_lora_wgrad(N.ptr(dd_dev), N.ptr(x[:, off:]), ld, m, pad, r, scale, N.ptr(g), sr, sk,
                                              N.ptr(col_map), N.ptr(scratch), N.stream_ptr()))
                    sync()
                # dA form: G [r][k], zeroed
                z = torch.zeros(r, k, device=DEV)
                run(z, k, 1)
                err = (z.cpu().double() - ref).abs()
                bound = m * U * terms_abs + 1e-30
                assert bool((err <= bound).all()), (lay, m, r, ld, float((err / bound).max()))
                z2 = torch.zeros(r, k, device=DEV)
                run(z2, k, 1)
                assert torch.equal(z, z2), "two runs differ"
                # dB form: G [k][r] (strides 1, r): the same numbers, transposed
                zt = torch.zeros(k, r, device=DEV)
                run(zt, 1, r)
                assert torch.equal(zt.t(), z)
                # accumulation into a non-zero G at every fp32 alignment, with a scale
                zs = torch.zeros(r, k, device=DEV)
                run(zs, k, 1, 0.5)
                for shift in (0, 1, 2, 3):
                    buf = torch.zeros(r * k + 8, device=DEV)
                    g0 = det("lora.wg.g0.%s.%d" % (lay, r), (r, k)).to(DEV)
                    g = buf[shift:shift + r * k].view(r, k)
                    g.copy_(g0)
                    assert g.data_ptr() % 16 == 4 * shift
                    run(g, k, 1, 0.5)
                    assert torch.equal(g, g0 + zs), (lay, m, r, shift)
                    assert float(buf[:shift].abs().sum()) == 0 and float(buf[shift + r * k:].abs().sum()) == 0


def test_wgrad_without_a_column_map():
    """col_map NULL: identity over all k columns"""
    L = N.lib()
    m, k, r = 65, 64, 4
    x = bf16_round(det("lora.wg.nomap.x", (m, k)))
    dd = det("lora.wg.nomap.d", (m, r))
    g = torch.zeros(r, k, device=DEV)
    scratch = torch.empty(L.ctta_lora_wgrad_scratch_floats(m, k, r), device=DEV)
    dd_dev, x_dev = dd.to(DEV), x.to(torch.bfloat16).to(DEV)
    N.check(L.ctta_lora_wgrad(N.ptr(dd_dev), N.ptr(x_dev), k, m, k, r, 1.0, N.ptr(g), k, 1, None, N.ptr(scratch),
                              N.stream_ptr()))
    sync()
    ref = dd.double().t() @ x.double()
    assert bool(((g.cpu().double() - ref).abs() <= m * U * (dd.double().abs().t() @ x.double().abs()) + 1e-30).all())


def test_bad_arguments_are_refused():
    L = N.lib()
    t = torch.zeros(64, 64, dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(64 * 64, device=DEV)
    assert L.ctta_lora_down(N.ptr(t), 64, 4, 64, N.ptr(f), 0, 17, N.ptr(f), N.stream_ptr()) != 0       # rank
    assert L.ctta_lora_down(N.ptr(t), 60, 4, 60, N.ptr(f), 0, 4, N.ptr(f), N.stream_ptr()) != 0        # width not a multiple of 8
    assert L.ctta_lora_down(N.ptr(t), 32, 4, 64, N.ptr(f), 0, 4, N.ptr(f), N.stream_ptr()) != 0        # ld < k
    assert L.ctta_lora_up_add(N.ptr(t[0, 1:]), 64, 4, 56, N.ptr(f), N.ptr(f), 0, 4, 1.0, N.stream_ptr()) != 0   # alignment
    assert L.ctta_lora_wgrad_scratch_floats(10, 60, 4) == 0 and L.ctta_lora_wgrad_scratch_floats(10, 64, 0) == 0
