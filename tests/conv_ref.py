"""Float64 reference of one ctta_conv_desc, input families, per-element bounds, a mirror of the kernel's per-wave epilogue
choice and the case table of the conv_gemm forward (csrc/conv_gemm_kernel.h, conv_epilogue.h, conv_plan.hip).  No GPU call at
import: test_conv_ref_cpu.py checks this module on the CPU, test_conv_forms_gpu.py uses it against the kernels.

Layouts are the kernel's: x is NHWC (B, hs, ws, x_stride) BEFORE the x2 upsample, a weight row is (kh, kw, c)-ordered and
k_pad long, the GEMM result is (M, n) with M = B * ho * wo; element (m, j) of group g leaves at flat output index
dest_index()[g, m, j] (-1: clipped by out_limit).

Value, per element:   tot = alpha * (sum + bias + rowvec + bias_m + res [+ old out]),  val = act(tot),
                      out = bf16(val) or fp32(val),  out2 = bf16(leaky(bf16(val))),  GEGLU: val = tot_value * gelu(tot_gate).
Bound, per element (families `uniform` and `offset`):
  delta = Lip(act) * 2^-24 * (L * A + |tot|) (+ 2 * 2^-24 |val| with an activation: its own roundings)
  bf16 outputs  2^-8 (|val| + delta) + delta          fp32 outputs  delta (+ TANH_F32_ABS behind a tanh)
  A   the same expression as tot over absolute values,
  L   the fp32 roundings on the longest path to the element, as the kernel is written:
        ceil(k_pad / 8) + 8   the K walk: every 16x16x32 MFMA read as four chained 8-term stages (the model of wgrad_ref.py:
                              one rounding per stage on the chain, 8 inside the stage that holds the largest term); the walk
                              is at most k_pad terms long whatever BK, and zero terms round nothing;
        + parts               two-pass split-K: `splits` slabs added by the finish pass; stream-K: the most parts any tile of
                              the launch is cut into (sk_max_parts, from the kernel's own partition); 0 otherwise;
        + 5                   the epilogue's additions: (bias + rowvec), + acc, + bias_m, + res, + old out;
        + 2                   the scale by alpha and the LeakyReLU product.
  Lip 1 (none, LeakyReLU with a slope in [0, 1], tanh), 1.1 (SiLU: max |d/dx x sigmoid(x)| = 1.0998), GEGLU: see bound().
  bf16 x bf16 products are exact in fp32.
Families `integer` and `impulse`: no bound.  Every fp32 partial sum is an integer below 2^24 and the result is a bf16 number,
so the kernel must give the reference BIT FOR BIT in any summation order, split or not (test_conv_ref_cpu.py proves both
conditions from the table for every case that lists the family).
"""
import ctypes
import math

import numpy as np
import torch

from consistencytta_amd import _native as N
from consistencytta_amd import spec

EPS24 = 2.0 ** -24
# Worst |tanhf(x) - tanh(x)| of the device's tanhf on fp32 outputs, doubled: this ROCm ships no accuracy table for its device
# math functions, so the figure is measured (LABNOTES.md XXII: 1.53e-7 is the worst |stored - float64 reference| over the scalar-
# store tanh cases of the table, the K walk's own error included: an upper bound of the function's.  A small sample -- 3 tiles x
# 286 rows x 2 families = 1716 arguments, |x| < 3 on `uniform`, saturated on `offset` -- for a term that is 1 % of L A 2^-24 there).
TANH_F32_ABS = 2 * 1.6e-7
# gelu_erf_f (csrc/common.h) states |error of erf| <= 1.5e-7 (Abramowitz-Stegun 7.1.26): Phi is half of it, times |g| <= 8
GELU_PHI_ABS = 1.0e-7
SENTINEL = 12288.0            # bf16- and fp32-representable, far outside every case's value range

# The environment every case is planned under: test_conv_plan_cpu.py's ENV0 (one MI355X, default options, the default workspace)
ENV0 = dict(cu_count=256, xcd=1, splitk=1, streamk=1, streamk_grid=0, suppress_splitk=0, stamps_bound=0,
            workspace_bytes=192 << 20, workspace_header_zeroed=1)
PTRS = ("x0", "x1", "w", "bias", "bias_m", "rowvec", "res", "out", "out2", "gn_part")
PLAN_FIELDS = [f for f, _ in N.ConvPlanInfo._fields_]


def rup(a, b):
    return (a + b - 1) // b * b


def det(name, shape, seed=0):
    return torch.from_numpy(spec.det_uniform(name, tuple(shape), seed))


def bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


def f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------ cases
def _case(id, cls, B=2, hs=13, ws=11, c0=64, n=72, **kw):
    c = dict(id=id, cls=tuple(cls), B=B, hs=hs, ws=ws, ups=0, c0=c0, c1=0, xs=0, kh=1, kw=1, sh=1, sw=1, ph=0, pw=0, dh=1, dw=1,
             ho=None, wo=None, n=n, n_rows=None, ldc=None, groups=1, bias=0, bias_m=0, rowvec=0, res=0, acc=0, alpha=0,
             out_act=0, out2=0, out_f32=0, in_act=0, strided=None, gn=0, tile=0, ws_bind=0, k_pad=None,
             families=("uniform", "integer", "impulse"))
    c.update(kw)
    hi, wi = (2 * c["hs"], 2 * c["ws"]) if c["ups"] else (c["hs"], c["ws"])
    c["hi"], c["wi"] = hi, wi
    if c["ho"] is None:
        c["ho"] = (hi + 2 * c["ph"] - c["dh"] * (c["kh"] - 1) - 1) // c["sh"] + 1
    if c["wo"] is None:
        c["wo"] = (wi + 2 * c["pw"] - c["dw"] * (c["kw"] - 1) - 1) // c["sw"] + 1
    c["M"] = c["B"] * c["ho"] * c["wo"]
    c["ct"] = c["c0"] + c["c1"]
    c["K"] = c["kh"] * c["kw"] * c["ct"]
    if c["k_pad"] is None:
        c["k_pad"] = rup(c["K"], 64)
    if c["n_rows"] is None:
        c["n_rows"] = c["n"] + 3
    if c["ldc"] is None:
        c["ldc"] = (c["n"] // 2 if c["out_act"] == 4 else rup(c["n"], 4)) + 8
    if c["xs"] == 0:
        c["xs"] = c["c0"] if c["groups"] == 1 else c["groups"] * c["c0"] + 8
    c["xgs"] = c["c0"] if c["groups"] > 1 else 0
    c["wgs"] = c["n_rows"] * c["k_pad"] if c["groups"] > 1 else 0
    c["ogs"] = c["M"] * c["ldc"] + 16 if c["groups"] > 1 else 0
    fams = tuple(f for f in c["families"] if not (f in ("integer", "impulse") and c["out_act"] in (1, 2, 4)))
    if c["acc"] or c["res"] or c["rowvec"] or c["bias_m"] or c["alpha"]:
        fams = tuple(f for f in fams if f != "impulse")          # impulse: no epilogue
    c["families"] = fams
    return c


def slopes(family):
    """in_slope, out_slope, out2_slope, alpha (when the case scales): the production slopes; powers of two on `integer`."""
    if family in ("integer", "impulse"):
        return dict(in_slope=0.5, out_slope=0.25, out2_slope=0.125, alpha=0.5)
    return dict(in_slope=f32(0.1), out_slope=f32(0.01), out2_slope=f32(0.1), alpha=f32(0.3))


def desc_fields(c, family="uniform"):
    """The ctta_conv_desc of a case; pointer fields 1 = bound / 0 = NULL (the GPU file puts the addresses in)."""
    s = slopes(family)
    st = c["strided"] or {}
    d = dict(x0=1, c0=c["c0"], x1=int(c["c1"] > 0), c1=c["c1"], batch=c["B"], hi=c["hi"], wi=c["wi"], upsample=c["ups"],
             ho=c["ho"], wo=c["wo"], kh=c["kh"], kw=c["kw"], stride_h=c["sh"], stride_w=c["sw"], pad_h=c["ph"], pad_w=c["pw"],
             dil_h=c["dh"], dil_w=c["dw"], w=1, k_pad=c["k_pad"], n=c["n"], bias=c["bias"], bias_m=c["bias_m"],
             rowvec=c["rowvec"], rowvec_ld=c["n"] + 4 if c["rowvec"] else 0, res=c["res"], res_ld=c["n"] + 4 if c["res"] else 0,
             in_act=c["in_act"], in_slope=s["in_slope"], out_act=c["out_act"], out_slope=s["out_slope"],
             alpha=s["alpha"] if c["alpha"] else 1.0, accumulate=c["acc"], out=1, ldc=c["ldc"], out_f32=c["out_f32"],
             out2=c["out2"], out2_slope=s["out2_slope"], out_batch_stride=st.get("obs", 0), out_offset=st.get("off", 0),
             out_limit=st.get("lim", 0), groups=c["groups"], x_group_stride=c["xgs"], w_group_stride=c["wgs"],
             out_group_stride=c["ogs"], tile=c["tile"], x_stride=c["xs"] if c["xs"] != c["c0"] else 0,
             gn_part=int(c["gn"] > 0), gn_groups=c["gn"], gn_hw=c["ho"] * c["wo"] if c["gn"] else 0,
             gn_part_floats=1 << 20 if c["gn"] else 0)
    return d


def make_desc(fields, ptrs=None):
    d = N.ConvDesc()
    for k, v in fields.items():
        if k in PTRS:
            v = ((ptrs or {}).get(k, 0x1000) if v else None)
        setattr(d, k, v)
    return d


def plan(lib, c, family="uniform"):
    """(status, ctta_conv_plan_info as a dict, or the error text) under ENV0."""
    out = N.ConvPlanInfo()
    st = lib.ctta_conv_plan(ctypes.byref(make_desc(desc_fields(c, family))), ctypes.byref(N.ConvPlanEnv(**ENV0)), ctypes.byref(out))
    if st:
        return st, lib.ctta_last_error().decode()
    return 0, {f: getattr(out, f) for f in PLAN_FIELDS}


def tile_geom(lib, vid):
    """dict(bm, bn, bk, wm, wn, mode, stages, sk) from ctta_conv_gemm_variant_name: 'BMxBNxBK_wWMxWN_mMODE_sSTAGES[_sk]'."""
    name = lib.ctta_conv_gemm_variant_name(vid).decode()
    parts = name.split("_")
    bm, bn, bk = (int(v) for v in parts[0].split("x"))
    wm, wn = (int(v) for v in parts[1][1:].split("x"))
    g = dict(name=name, bm=bm, bn=bn, bk=bk, wm=wm, wn=wn, mode=int(parts[2][1:]), stages=int(parts[3][1:]), sk=len(parts) > 4)
    g["tm"], g["tn"] = bm // wm, bn // wn
    g["frags"] = (g["tm"] // 16) * (g["tn"] // 16)
    return g


# ------------------------------------------------------------------------------------------------ inputs
def impulse_sites(c):
    """(b, h, w, channel) of the impulses: the four corners of sample 0, the last pixel of sample 0 and the first of the last
    sample, a pixel inside; channels: first, last, both sides of every 8-chunk edge that matters (7 | 8, c0 - 1 | c0 with a
    second source)."""
    B, H, W, ct = c["B"], c["hs"], c["ws"], c["ct"]
    flat = [(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (0, H - 1, W - 1), (B - 1, 0, 0), (B - 1, H - 1, W - 1), (0, H // 2, W // 2)]
    chans = [0, ct - 1, 7, 8 % ct, c["c0"] - 1, c["c0"] % ct, ct // 2]
    return [(b, h, w, chans[i % len(chans)]) for i, (b, h, w) in enumerate(flat)]


def make_inputs(c, family):
    """dict of fp32 CPU tensors holding bf16-representable values (bias / rowvec / bias_m: fp32 values):
    x (G, B, hs, ws, c0), x1 (B, hs, ws, c1) or None, w (G, n, K), bias (n), bias_m (M), rowvec (B, n), res (M, n), old (M, n)."""
    G, B, hs, ws, c0, c1, n, K, M = c["groups"], c["B"], c["hs"], c["ws"], c["c0"], c["c1"], c["n"], c["K"], c["M"]
    tag = "cv.%s" % c["id"]
    shp_x, shp_1, shp_w = (G, B, hs, ws, c0), (B, hs, ws, max(c1, 1)), (G, n, K)
    out = {}
    if family in ("uniform", "offset"):
        off = 0.0 if family == "uniform" else 1.5
        out["x"] = bf16_round(off + det(tag + ".x", shp_x, 1))
        out["x1"] = bf16_round(off + det(tag + ".x1", shp_1, 2))
        out["w"] = bf16_round((off + det(tag + ".w", shp_w, 3)) * (1.0 / math.sqrt(K)))
        out["bias"] = det(tag + ".b", (n,), 4) * 0.1
        out["bias_m"] = det(tag + ".bm", (M,), 5) * 0.5
        out["rowvec"] = det(tag + ".rv", (B, n), 6) + 3.0 * torch.arange(B).view(B, 1).float()       # >= 1 apart between samples
        out["res"] = bf16_round(det(tag + ".res", (M, n), 7))
        out["old"] = bf16_round(det(tag + ".old", (M, n), 8))
    elif family == "integer":
        share = min(1.0, 576.0 / K)          # thin w as K grows: |sum| stays near 150 (bf16 holds integers up to 256)
        out["x"] = torch.round(det(tag + ".x", shp_x, 1) * 2.49)
        out["x1"] = torch.round(det(tag + ".x1", shp_1, 2) * 2.49)
        keep = (det(tag + ".wk", shp_w, 9).abs() < share).float()
        out["w"] = torch.round(det(tag + ".w", shp_w, 3) * 1.49) * keep
        out["bias"] = torch.round(det(tag + ".b", (n,), 4) * 3.49)
        if c["gn"]:
            # GroupNorm cases: every value is an integer + 1/64 -- exact in fp32, mostly NOT a bf16 number, and the sum of a
            # partial's values is exact in fp32 in any order (test_conv_ref_cpu.py: 64 * sum |v| < 2^24): the sums of the
            # unrounded values have ONE right answer, and the sums of the stored values are far from it
            out["bias"] = out["bias"] + 0.015625
        out["bias_m"] = torch.round(det(tag + ".bm", (M,), 5) * 2.49)
        out["rowvec"] = torch.round(det(tag + ".rv", (B, n), 6) * 2.49) + 5.0 * (torch.arange(B).view(B, 1) % 3).float()
        out["res"] = torch.round(det(tag + ".res", (M, n), 7) * 3.49)
        out["old"] = torch.round(det(tag + ".old", (M, n), 8) * 3.49)
    else:
        assert family == "impulse"
        x, x1 = torch.zeros(shp_x), torch.zeros(shp_1)
        for b, h, w_, ch in impulse_sites(c):
            if ch < c0:
                x[:, b, h, w_, ch] = 1.0
            else:
                x1[b, h, w_, ch - c0] = 1.0
        out["x"], out["x1"] = x, x1
        j, k = torch.arange(n).view(1, n, 1), torch.arange(K).view(1, 1, K)
        out["w"] = (((7 * j + 3 * k + 11 * torch.arange(G).view(G, 1, 1)) % 61) - 30).float()
        for key, shp in (("bias", (n,)), ("bias_m", (M,)), ("rowvec", (B, n)), ("res", (M, n)), ("old", (M, n))):
            out[key] = torch.zeros(shp)
    if c1 == 0:
        out["x1"] = None
    return out


# ------------------------------------------------------------------------------------------------ reference
def gather64(c, x, x1):
    """Q (M, K) float64: Q[m][tap * ct + ch] = source[pixel(m, tap)][ch], zero outside the (logical, upsampled) image.
    x (B, hs, ws, c0), x1 (B, hs, ws, c1) or None."""
    B, ho, wo, ct, c0 = c["B"], c["ho"], c["wo"], c["ct"], c["c0"]
    m = torch.arange(c["M"])
    b, rem = m // (ho * wo), m % (ho * wo)
    oh, ow = rem // wo, rem % wo
    q = torch.zeros(c["M"], c["K"], dtype=torch.float64)
    xs = x.double() if x1 is None else torch.cat([x.double(), x1.double()], dim=-1)
    for a in range(c["kh"]):
        for bq in range(c["kw"]):
            ih, iw = oh * c["sh"] - c["ph"] + a * c["dh"], ow * c["sw"] - c["pw"] + bq * c["dw"]
            ok = (ih >= 0) & (ih < c["hi"]) & (iw >= 0) & (iw < c["wi"])
            if c["ups"]:
                ih, iw = ih // 2, iw // 2
            v = xs[b, ih.clamp(0, c["hs"] - 1), iw.clamp(0, c["ws"] - 1)] * ok.view(-1, 1).double()
            t = a * c["kw"] + bq
            q[:, t * ct:(t + 1) * ct] = v
    return q


def _leaky(v, s):
    return torch.where(v > 0, v, v * s)


def _act(c, tot, s):
    if c["out_act"] == 1:
        return tot * torch.sigmoid(tot)
    if c["out_act"] == 2:
        return torch.tanh(tot)
    if c["out_act"] == 3:
        return _leaky(tot, s["out_slope"])
    return tot


def geglu_cols(n):
    """value and gate GEMM columns of hidden unit h (rows packed in 16-blocks [16 value][16 gate]), as
    test_linear_with_fused_geglu_epilogue packs them: h -> (h // 16) * 32 + h % 16, + 16."""
    h = torch.arange(n // 2)
    v = (h // 16) * 32 + h % 16
    return v, v + 16


def reference(c, inp, family):
    """dict: tot, A (G, M, n) float64 -- the value before the activation and the same expression over absolute values --
    val (G, M, cols): the value before the output rounding, cols = n (n / 2 with GEGLU, where tot / A keep the GEMM columns),
    sum (G, M, n): the bare products."""
    s = slopes(family)
    alpha = s["alpha"] if c["alpha"] else 1.0
    B, n, M = c["B"], c["n"], c["M"]
    bsel = torch.arange(M) // (c["ho"] * c["wo"])
    e = torch.zeros(M, n, dtype=torch.float64)
    ea = torch.zeros(M, n, dtype=torch.float64)
    for key, on, expand in (("bias", c["bias"], lambda t: t.view(1, n)), ("rowvec", c["rowvec"], lambda t: t[bsel]),
                            ("bias_m", c["bias_m"], lambda t: t.view(M, 1)), ("res", c["res"], lambda t: t),
                            ("old", c["acc"], lambda t: t)):
        if on:
            t = expand(inp[key].double())
            e, ea = e + t, ea + t.abs()
    tots, As, sums = [], [], []
    for g in range(c["groups"]):
        x = inp["x"][g]
        if c["in_act"]:
            x = bf16_round(_leaky(x, s["in_slope"]))
            assert inp["x1"] is None
        q = gather64(c, x, inp["x1"])
        w = inp["w"][g].double()
        sm = q @ w.t()
        sums.append(sm)
        tots.append(alpha * (sm + e))
        As.append(abs(alpha) * (q.abs() @ w.abs().t() + ea))
    tot, A = torch.stack(tots), torch.stack(As)
    if c["out_act"] == 4:
        vc, gc = geglu_cols(n)
        gate = tot[..., gc]
        val = tot[..., vc] * (gate * 0.5 * (1.0 + torch.erf(gate / math.sqrt(2.0))))
    else:
        val = _act(c, tot, s)
    return dict(tot=tot, A=A, val=val, sum=torch.stack(sums))


def expected_out(c, ref, family):
    """(out, out2) as the kernel must store them when its arithmetic is exact (families integer / impulse): fp32 tensors."""
    val = ref["val"].float()
    out = val if c["out_f32"] else bf16_round(val)
    out2 = bf16_round(_leaky(bf16_round(val), slopes(family)["out2_slope"])) if c["out2"] else None
    return out, out2


def dest_index(c):
    """(G, M, cols) int64: flat element index of every result in the output buffer, -1 where out_limit clips it."""
    G, M = c["groups"], c["M"]
    cols = c["n"] // 2 if c["out_act"] == 4 else c["n"]
    m, j = torch.arange(M).view(M, 1), torch.arange(cols).view(1, cols)
    st = c["strided"]
    if st:
        howo = c["ho"] * c["wo"]
        b = m // howo
        inb = (m - b * howo) * c["ldc"] + j + st["off"]
        ok = (inb >= 0) & (inb < st["lim"]) if st["lim"] > 0 else torch.ones_like(inb, dtype=torch.bool)
        idx = torch.where(ok, b * st["obs"] + inb, torch.full_like(inb, -1))
    else:
        idx = m * c["ldc"] + j
    g = torch.arange(G).view(G, 1, 1) * c["ogs"]
    return torch.where(idx.unsqueeze(0) >= 0, idx.unsqueeze(0) + g, torch.full((G, M, cols), -1, dtype=torch.int64))


def out_elems(c):
    """elements of the output allocation (guard bands not counted)"""
    if c["strided"]:
        return c["B"] * c["strided"]["obs"]
    return (c["groups"] - 1) * c["ogs"] + c["M"] * c["ldc"]


# ------------------------------------------------------------------------------------------------ bound
def sk_max_parts(pl):
    """The most parts a tile of a stream-K launch is cut into: conv_gemm_sk_kernel's tile_parts over every chunk."""
    G, nch, nk = pl["grid_x"], max(pl["sk_chunks"], 1), pl["nk"]
    T = pl["m_tiles"] * pl["n_tiles"]
    per, worst = G // nch, 1
    for ch in range(nch):
        lo, hi = ch * T // nch, (ch + 1) * T // nch
        items = (hi - lo) * nk
        for tl in range(hi - lo):
            first = ((tl * nk + 1) * per - 1) // items
            last = ((tl + 1) * nk * per - 1) // items
            worst = max(worst, last - first + 1)
    return worst


def L_of(c, pl):
    parts = pl["splits"] if pl["splits"] > 1 else sk_max_parts(pl) if pl["kind"] == 2 else 0
    return -(-c["k_pad"] // 8) + 8 + parts + 5 + 2


def bound(c, ref, pl):
    """Per-element bound on |stored - val| (module docstring), (G, M, cols) float64."""
    L = L_of(c, pl)
    tot, A, val = ref["tot"], ref["A"], ref["val"].abs()
    d = EPS24 * (L * A + tot.abs())
    if c["out_act"] == 4:
        # val = v * g * Phi(g): |d val| <= |g Phi(g)| d_v + |v| * max|d/dg g Phi(g)| (= 1.13) d_g + |v g| GELU_PHI_ABS, + 3 roundings
        vc, gc = geglu_cols(c["n"])
        v, g = tot[..., vc], tot[..., gc]
        gel = g * 0.5 * (1.0 + torch.erf(g / math.sqrt(2.0)))
        d = gel.abs() * d[..., vc] + v.abs() * (1.13 * d[..., gc] + g.abs() * GELU_PHI_ABS) + 3 * EPS24 * val
    elif c["out_act"] in (1, 2):
        d = (1.1 if c["out_act"] == 1 else 1.0) * d + 2 * EPS24 * val
    if c["out_f32"]:
        return d + (TANH_F32_ABS if c["out_act"] == 2 else 0.0)
    return 2.0 ** -8 * (val + d) + d


def worst_ratio(err, bnd):
    """max err / bound; an element with bound 0 must have error 0 (inf otherwise)."""
    err, bnd = err.double().reshape(-1), bnd.double().reshape(-1)
    if err.numel() == 0:
        return 0.0
    r = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    r = torch.where(torch.isfinite(err), r, torch.full_like(err, math.inf))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ which code wrote an element
ROUTES = ("halo", "finish_wide4", "finish_store", "streamk", "wide_f32", "geglu_fast", "geglu_wide4", "geglu_direct", "fast", "fast_str",
          "wide4_edge", "wide4_sample", "wide4_str", "wide4", "store")


def wave_routes(c, pl, geom, tail_geom=None):
    """(M, n) tensor of indices into ROUTES: the epilogue code that writes element (m, j), by the kernel's own per-wave
    predicate (conv_tile, `fast_wave`):   epi_fast  and  n0 + wn * TN + TN <= n
                                          and (no rowvec or the TILE's rows below M lie in one sample)
                                          and (plain destination or the WAVE's rows below M lie in one sample).
    Rows of the cut-off tail launch are judged with the tail tile's geometry and m_off."""
    M, n, howo = c["M"], c["n"], c["ho"] * c["wo"]
    R = {k: i for i, k in enumerate(ROUTES)}
    out = torch.full((M, n), -1, dtype=torch.int64)
    if pl["halo"]:
        return out.fill_(R["halo"])
    if pl["splits"] > 1:
        return out.fill_(R["finish_wide4" if pl["wide_store"] else "finish_store"])
    if pl["kind"] == 2:
        return out.fill_(R["streamk"])
    if pl["wide_f32"]:
        return out.fill_(R["wide_f32"])
    if not pl["wide_store"]:          # MFMA-layout stores: epilogue_store, or epilogue_geglu (GEGLU with a destination that is not plain)
        return out.fill_(R["geglu_direct" if c["out_act"] == 4 else "store"])
    m, j = torch.arange(M).view(M, 1), torch.arange(n).view(1, n)

    def region(g, m_lo, m_hi):
        mm = m[m_lo:m_hi] - m_lo
        m0 = m_lo + mm // g["bm"] * g["bm"]
        mw = m0 + (mm % g["bm"]) // g["tm"] * g["tm"]
        col_in = (j // g["tn"] * g["tn"] + g["tn"] <= n).expand(m_hi - m_lo, n)
        tile_one = (m0 // howo == (torch.minimum(m0 + g["bm"], torch.tensor(M)) - 1) // howo).expand(-1, n)
        wave_one = (mw // howo == (torch.minimum(mw + g["tm"], torch.tensor(M)) - 1) // howo).expand(-1, n)
        if c["out_act"] == 4:
            r = torch.where(col_in if pl["epi_fast_geglu"] else torch.zeros_like(col_in), R["geglu_fast"], R["geglu_wide4"])
        elif not pl["epi_fast"]:
            r = torch.full((m_hi - m_lo, n), R["wide4"])
        else:
            r = torch.full((m_hi - m_lo, n), R["fast" if pl["plain_out"] else "fast_str"])
            if not pl["plain_out"]:
                r = torch.where(wave_one, r, torch.tensor(R["wide4_str"]))
            if c["rowvec"]:
                r = torch.where(tile_one, r, torch.tensor(R["wide4_sample"]))
            r = torch.where(col_in, r, torch.tensor(R["wide4_edge"]))
        out[m_lo:m_hi] = r

    cut = M - pl["tail_rows"]
    region(geom, 0, cut)
    if pl["tail_rows"]:
        region(tail_geom, cut, M)
    return out


# ------------------------------------------------------------------------------------------------ GroupNorm partials
def gn_reference(c, ref, pl, geom):
    """The contract of ctta_conv_desc.gn_part (include/ctta.h): (sum, sum of squares) of the fp32 values BEFORE the bf16
    rounding.  -> s (B, nchunk, G, 2) float64, the same over absolute values / a (B, nchunk, G), the element count per entry.
    chunk = ((row tile in the sample) * WM + wave row) * SUB + column slice of a group wider than a wave's TN columns."""
    B, n, G, hw = c["B"], c["n"], c["gn"], c["ho"] * c["wo"]
    cpg, tn, tm, bm, wm = n // G, geom["tn"], geom["tm"], geom["bm"], geom["wm"]
    cw = min(cpg, tn)
    sub = cpg // cw
    nchunk = hw // bm * wm * sub
    v = ref["val"][0].view(B, hw // tm, tm, G, sub, cw)          # rows: (sample, wave-row block), columns: (group, slice)
    s1 = v.sum(dim=(2, 5)).permute(0, 1, 3, 2)                   # (B, blocks, sub, G)
    s2 = (v * v).sum(dim=(2, 5)).permute(0, 1, 3, 2)
    a1 = v.abs().sum(dim=(2, 5)).permute(0, 1, 3, 2)
    shp = (B, nchunk, G)
    return torch.stack([s1.reshape(shp), s2.reshape(shp)], dim=-1), a1.reshape(shp), tm * cw


def gn_bound(c, ref, pl, geom):
    """|partial - float64 sum| per entry: the elements' own errors (delta each, 2 |v| delta on the squares) plus the fp32
    additions of the fold, terms = a lane's elements (TM * cw / 64 ... at most TM * TN / 64) + the butterfly's 6 + 2."""
    B, n, G, hw = c["B"], c["n"], c["gn"], c["ho"] * c["wo"]
    cpg, tn, tm = n // G, geom["tn"], geom["tm"]
    cw = min(cpg, tn)
    sub = cpg // cw
    d = EPS24 * (L_of(c, pl) * ref["A"][0] + ref["tot"][0].abs())
    v = ref["val"][0]
    terms = tm * tn // 64 + 8

    def fold(t):
        return t.view(B, hw // tm, tm, G, sub, cw).sum(dim=(2, 5)).permute(0, 1, 3, 2).reshape(B, -1, G)

    b1 = fold(d) + EPS24 * terms * fold(v.abs())
    b2 = fold(2 * v.abs() * d + d * d) + EPS24 * (terms + 1) * fold(v * v)
    return torch.stack([b1, b2], dim=-1)


# ------------------------------------------------------------------------------------------------ the case table
MODE2_IDS = tuple(list(range(17, 25)) + list(range(26, 44)))
BK32_IDS = (2, 10, 18, 25, 26, 28, 30, 32, 33, 34, 35)
SK_IDS = (41, 42, 43)
EPI_TILES = (21, 17, 29)          # a small-fragment tile (4), a 16-fragment tile, an 8-wave tile (32 fragments per wave)
FULL = dict(bias=1, rowvec=1, res=1)


def _tile_cases():
    """List 1: every tile id forced, ragged in M (286 = 2 x 13 x 11 rows) and in N (72: n % TN = 8 for TN = 32 and 64), with
    bias + rowvec + res, so that a launch has straight-line waves, column-edge waves and (143 rows per sample) tiles that
    straddle two samples."""
    out = []
    k3 = dict(kh=3, kw=3, ph=1, pw=1)
    fam2 = ("uniform", "integer")
    for t in list(range(1, 17)) + [25]:
        out.append(_case("t%d-c40" % t, ["tile", "tile:c40"], c0=40, tile=t, families=fam2, **k3, **FULL))
        out.append(_case("t%d-cat" % t, ["tile", "tile:concat"], c0=64, c1=40, tile=t, families=fam2, **k3, **FULL))
    for t in range(1, 17):
        out.append(_case("t%d-c40-plain" % t, ["tile", "tile:c40"], c0=40, tile=t, bias=1, families=("impulse",), **k3))
    for t in MODE2_IDS:
        if t in SK_IDS:
            continue
        big = dict(hs=25, ws=24) if t in (35, 36) else {}          # 512-row tiles: 600 rows per sample, so that tile 0 lies in one
        out.append(_case("t%d-c64" % t, ["tile", "tile:ct%bk==0"], c0=64, tile=t, families=fam2, **big, **k3, **FULL))
        out.append(_case("t%d-c64-plain" % t, ["tile", "tile:ct%bk==0"], c0=64, tile=t, bias=1, families=("impulse",), **k3))
    for t in BK32_IDS:
        big = dict(hs=25, ws=24) if t == 35 else {}
        out.append(_case("t%d-c96" % t, ["tile", "tile:bk32:c96"], c0=96, tile=t, families=fam2, **big, **k3, **FULL))
    for t in SK_IDS:          # the shapes of test_conv3x3_all_tiles (M = 768) and test_conv_geometries_on_streamk_tiles (M = 2560)
        out.append(_case("t%d-sk-M768" % t, ["tile", "tile:sk:M768", "sched:streamk"], B=2, hs=24, ws=16, c0=64, n=96, tile=t,
                         ws_bind=1, families=("uniform", "integer", "impulse"), bias=1, **k3))
        out.append(_case("t%d-sk-M2560" % t, ["tile", "tile:sk:M2560", "sched:streamk"], B=5, hs=32, ws=16, c0=128, n=320, tile=t,
                         ws_bind=1, families=fam2, **k3, **FULL))
    return out


GATHER_TILES = (5, 13, 21)        # 64x64x64 in staging modes 0, 1, 2


def _gather_cases():
    """List 2: gather classes on one tile of each staging mode; n = 40 (TN = 32: a column-edge wave), no epilogue."""
    G = []

    def add(name, refuse2=False, only0=False, families=("uniform", "integer", "impulse"), **kw):
        for mode, t in enumerate(GATHER_TILES):
            c = _case("g-%s-m%d" % (name, mode), ["gather:%s" % name, "gather:%s:m%d" % (name, mode)], n=40, tile=t,
                      families=families, **kw)
            if mode == 2 and refuse2:
                c["refused"] = "needs (c0+c1) % BK == 0"
            if mode > 0 and only0:
                c["refused"] = "in_act needs a register-staged variant"
            G.append(c)

    add("3x3-pad1", B=2, hs=6, ws=5, kh=3, kw=3, ph=1, pw=1)
    add("3x3-pad0", B=2, hs=6, ws=5, kh=3, kw=3)
    add("3x3-pad2-dgrad", B=2, hs=6, ws=5, kh=3, kw=3, ph=2, pw=2)
    add("stride2", B=2, hs=9, ws=8, kh=3, kw=3, ph=1, pw=1, sh=2, sw=2)
    add("1xk-dil3", B=2, hs=1, ws=37, kw=7, pw=9, dw=3)
    add("1xk-dil5", B=2, hs=1, ws=37, kw=5, pw=10, dw=5)
    add("1x1", B=1, hs=9, ws=7)
    add("1x16", B=2, hs=1, ws=21, kw=16, pw=8)
    add("1x32", B=2, hs=1, ws=21, kw=32, pw=16)
    add("ups3x3", B=2, hs=3, ws=4, ups=1, kh=3, kw=3, ph=1, pw=1)
    add("width1", B=3, hs=5, ws=1, kh=3, kw=3, ph=1, pw=1)
    add("width2", B=3, hs=5, ws=2, kh=3, kw=3, ph=1, pw=1)
    add("width3", B=3, hs=5, ws=3, kh=3, kw=3, ph=1, pw=1)
    add("wo1", B=3, hs=7, ws=3, kh=3, kw=3, ph=1, pw=0)                      # wo = 1: wo_inv = 0xFFFFFFFF
    add("howo1", B=70, hs=1, ws=1, kh=3, kw=3, ph=1, pw=1)                   # howo = 1: both reciprocals, two row tiles
    add("x_stride", B=2, hs=6, ws=5, kh=3, kw=3, ph=1, pw=1, xs=88)
    add("groups3", B=1, hs=70, ws=1, groups=3, families=("uniform", "integer"))
    add("in_act", only0=True, B=2, hs=6, ws=5, kh=3, kw=3, ph=1, pw=1, in_act=1, families=("uniform", "integer"))
    # what MODE 2 refuses
    add("concat", refuse2=True, B=2, hs=6, ws=5, c0=64, c1=64, kh=3, kw=3, ph=1, pw=1)
    add("c40", refuse2=True, B=2, hs=6, ws=5, c0=40, kh=3, kw=3, ph=1, pw=1)
    add("1x33", refuse2=True, B=2, hs=1, ws=21, kw=33, pw=16)
    add("ups5x5", refuse2=True, B=2, hs=3, ws=4, ups=1, kh=5, kw=5, ph=2, pw=2)
    return G


def _schedule_cases():
    """List 3.  The plan fields that define a class are asserted in test_conv_ref_cpu.py."""
    f2 = ("uniform", "integer")
    k3 = dict(kh=3, kw=3, ph=1, pw=1)
    return [
        _case("s-xcd-n_inner1", ["sched:xcd:n_inner=1"], B=1, hs=4096, ws=1, c0=64, n=72, tile=21, bias=1, families=f2),
        _case("s-xcd-n_inner0", ["sched:xcd:n_inner=0"], B=1, hs=4096, ws=1, c0=1024, n=1088, tile=21, bias=1, families=("integer",)),
        _case("s-xcd-padding", ["sched:xcd:padding"], B=1, hs=64 * 66, ws=1, c0=64, n=72, tile=21, bias=1, families=f2),
        _case("s-slab-unsplit", ["sched:slab"], B=2, hs=8, ws=9, c0=128, n=520, tile=21, families=f2, **k3, **FULL),
        _case("s-splitk-full", ["sched:splitk", "sched:splitk:full"], B=1, hs=4, ws=5, c0=256, n=72, out_act=3, alpha=1, out2=1,
              families=f2, **k3, **FULL),
        _case("s-splitk-f32", ["sched:splitk", "sched:splitk:f32"], B=1, hs=4, ws=5, c0=256, n=72, out_f32=1, bias=1, families=f2, **k3),
        _case("s-splitk-t10", ["sched:splitk", "sched:splitk:not-wide-f32"], B=1, hs=4, ws=5, c0=256, n=72, tile=10, families=f2,
              **k3, **FULL),
        _case("s-splitk-t18", ["sched:splitk", "sched:splitk:not-wide-f32"], B=1, hs=4, ws=5, c0=256, n=72, tile=18, families=f2,
              **k3, **FULL),
        _case("s-splitk-ragged", ["sched:splitk", "sched:splitk:nk%splits"], B=1, hs=4, ws=5, c0=264, n=72, families=f2, **k3, **FULL),
        _case("s-halo", ["sched:halo"], B=2, hs=1, ws=300, c0=32, n=32, kw=7, pw=9, dw=3, bias=1),
        _case("s-tail", ["sched:tail"], B=1, hs=1, ws=65568, c0=64, n=256, kw=9, pw=4, bias=1, families=("integer",)),
    ]


def _epilogue_cases():
    """List 4: every epilogue class on a small-fragment tile, a 16-fragment tile and an 8-wave tile (EPI_TILES)."""
    out = []
    k3 = dict(kh=3, kw=3, ph=1, pw=1)
    f2 = ("uniform", "offset", "integer")
    classes = [
        ("bias", dict(bias=1)),
        ("rowvec", dict(bias=1, rowvec=1)),
        ("res", dict(bias=1, res=1)),
        ("res+out2", dict(bias=1, res=1, out2=1)),
        ("acc", dict(bias=1, acc=1)),
        ("acc+res+lrelu+alpha", dict(bias=1, acc=1, res=1, out_act=3, alpha=1)),
        ("bias_m", dict(bias=1, bias_m=1)),
        ("silu", dict(bias=1, res=1, out_act=1)),
        ("tanh", dict(bias=1, out_act=2)),
        ("f32-wide", dict(bias=1, out_f32=1)),
        ("f32-not-wide", dict(bias=1, res=1, out_f32=1, out_act=3)),
        ("scalar-ldc1", dict(bias=1, n=1, ldc=1, out_f32=1, out_act=2)),
        ("scalar-ldc3", dict(bias=1, bias_m=1, n=3, ldc=3)),
        ("plain-n%4", dict(n=70, ldc=76)),
    ]
    for name, kw in classes:
        for t in EPI_TILES:
            out.append(_case("e-%s-t%d" % (name, t), ["epi:%s" % name, "epi:%s:t%d" % (name, t)], tile=t, families=f2, **k3,
                             **kw))
    # fused GEGLU (a linear): n = 96 -> one column-edge wave on the TN = 64 tiles.  The 32-fragment tile is refused.
    for t in (21, 17, 28, 29):
        c = _case("e-geglu-t%d" % t, ["epi:geglu", "epi:geglu:t%d" % t], B=1, hs=150, ws=1, c0=64, n=96, out_act=4, bias=1, tile=t,
                  families=("uniform", "offset"))
        if t == 29:
            c["refused"] = "the fused GEGLU epilogue needs a tile"
        out.append(c)
    # ... and its direct, MFMA-layout form (epilogue_geglu): a destination that is not plain switches the wide store off, which
    # one sample with an out_batch_stride of its own does (the stride has nothing to act on).  The tiles with <= 8 fragments per
    # wave carry it: 64x64 (modes 0 and 2), 64x128, 128x64, 256x32, and what the rules pick (tile 0 -> 64x128x64); 150 rows and
    # n = 96 are ragged in every one of them but for N on 256x32.  A 16-fragment tile is refused.  With two samples the second
    # one starts at out_batch_stride, 64 elements behind the first one's last row.
    gst = dict(obs=150 * 56 + 64, off=0, lim=0)
    for t in (0, 5, 21, 22, 24, 20, 17):
        c = _case("e-geglu-direct-t%d" % t, ["epi:geglu-direct", "epi:geglu-direct:t%d" % t], B=1, hs=150, ws=1, c0=64, n=96, out_act=4,
                  bias=1, tile=t, ldc=56, strided=gst, families=("uniform", "offset"))
        if t == 17:
            c["refused"] = "the fused GEGLU epilogue needs a tile"
        out.append(c)
    c = _case("e-geglu-direct-B2", ["epi:geglu-direct"], B=2, hs=75, ws=1, c0=64, n=96, out_act=4, bias=1, tile=21, ldc=56,
              strided=dict(obs=75 * 56 + 64, off=0, lim=0), families=("uniform", "offset"))
    out.append(c)
    # strided, clipped destination (the ConvTranspose1d remap of test_conv_transpose1d_as_phase_gemm: u = 4 phases of 24
    # channels, k = 8: two taps, padding 2): 151 rows per sample, so that a 128-row wave lies inside a sample and the next one
    # straddles two; both ends of a sample are clipped
    u, co, L, taps, pad = 4, 24, 150, 2, 2
    Lout = (L - 1) * u - 2 * pad + 8
    Q = (Lout - 1 + pad) // u + 1
    st = dict(obs=Lout * co, off=-pad * co, lim=Lout * co)
    for name, kw in (("str", dict(bias=1)), ("str+out2+lrelu", dict(bias=1, out2=1, out_act=3, alpha=1))):
        for t in EPI_TILES:
            out.append(_case("e-%s-t%d" % (name, t), ["epi:%s" % name, "epi:%s:t%d" % (name, t)], B=3, hs=1, ws=L, wo=Q, c0=64,
                             kw=taps, pw=taps - 1, n=u * co, ldc=u * co, strided=st, tile=t, families=f2, **kw))
    # GroupNorm partials: 16 x 16 pixels per sample (a multiple of every BM), channels per group below / equal to / above TN
    for t, n, gs in ((21, 64, (4, 2, 1)), (17, 128, (4, 2, 1)), (29, 256, (8, 4, 2))):
        for G, rel in zip(gs, ("below", "equal", "above")):
            for res in (0, 1):
                out.append(_case("e-gn-%s%s-t%d" % (rel, "-res" if res else "", t),
                                 ["epi:gn", "epi:gn:cpg-%s" % rel, "epi:gn:res=%d" % res, "epi:gn:t%d" % t], B=2, hs=16, ws=16,
                                 c0=64, n=n, ldc=n, gn=G, bias=1, res=res, tile=t, families=("uniform", "offset", "integer"), **k3))
    out.append(_case("e-gn-edge-t17", ["epi:gn", "epi:gn:column-edge"], B=2, hs=16, ws=16, c0=64, n=96, ldc=96, gn=6, bias=1,
                     res=1, tile=17, families=("uniform", "offset", "integer"), **k3))
    # partials behind alpha and a LeakyReLU: the statistics instantiations carry neither, so the whole launch leaves through
    # epilogue_wide4 (epi_fast = 0) and its sums -- the contract's "after alpha and the output activation"
    out.append(_case("e-gn-act-t17", ["epi:gn", "epi:gn:act"], B=2, hs=16, ws=16, c0=64, n=128, ldc=128, gn=8, bias=1, res=1,
                     out_act=3, alpha=1, tile=17, families=("uniform", "offset", "integer"), **k3))
    return out


CASES = _tile_cases() + _gather_cases() + _schedule_cases() + _epilogue_cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


def case_params():
    """(case, family) pairs of the numeric tests (cases the plan refuses have none)."""
    return [(c, f) for c in CASES if not c.get("refused") for f in c["families"]]
