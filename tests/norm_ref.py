"""Float64 references, input generators, error bounds, case tables and the dispatchers' predicates for the norm and softmax
kernels of csrc/norm_elem.hip and the matching section of csrc/backward.hip.  No GPU call in here: test_norm_ref_cpu.py
checks this module on the CPU, test_norm_forms_gpu.py uses it against the kernels.

Layouts are the kernels': GroupNorm tensors are NHWC, (B, hw, C); LayerNorm and softmax matrices are (rows, ld) with
`d` / `cols` true columns.  Every reference takes the bf16-rounded (or fp32) values the kernel is handed and works in float64.

Bounds (each stated once, below, with its derivation):
  fwd_bound          per element,  2^-8 |ref| + 2^-10 M
  stats_bounds       per (sample, group)
  emulation_bounds   per (sample, group), stats_out against the emulated summation order
  slab_bound         dx / dS, per row or slab,  2 * BF16_TOL * max|ref|
  softmax_bwd_bound  per element
  param_bound        dgamma / dbeta per column,  (n 2^-24 + 2^-20) sum|t|

What was MEASURED (on the CPU, test_norm_ref_cpu.py::test_emulated_statistics_stay_inside_a_quarter_of_the_bounds prints
it): the loss of gn_stats_emulated -- fp32 per-channel running sums, the fold over the group's channels as gn_group_fold
names it (fp32 up to 128 terms, fp64 beyond), fp64 over the chunks, or the single-launch form's per-thread sums where
gn_small_ok -- against the float64 statistics, worst (sample, group) of sample 0 of each row of GN_FWD_CASES.  rstd: relative;
mean: in units of its bound 2^-20 (|mean| + std).

  B  C    hw   G  | benign  rstd / mean  | offset(16) rstd / mean | offset(64) rstd / mean
  2  256 2048 32 |  6.6e-08 / 0.013  |  7.6e-06 / 0.000  |  9.7e-05 / 0.000  |
  2  256 2049 32 |  4.8e-08 / 0.014  |  1.2e-05 / 0.023  |  1.6e-04 / 0.027  |
  2   40   45  8 |  3.7e-08 / 0.010  |  5.8e-08 / 0.033  |  4.4e-08 / 0.056  |
  1  320  300 32 |  7.3e-08 / 0.016  |  1.8e-05 / 0.053  |  2.2e-04 / 0.030  |
  1 2560  208 32 |  8.1e-08 / 0.011  |  1.2e-05 / 0.058  |  2.1e-04 / 0.029  |
  2 2048 1031 32 |  5.1e-08 / 0.012  |  4.2e-06 / 0.056  |  8.2e-05 / 0.031  |
  1  192  700 24 |  5.9e-08 / 0.013  |  5.7e-06 / 0.057  |  7.9e-05 / 0.030  |
  1  240 1000 24 |  7.5e-08 / 0.014  |  1.4e-05 / 0.057  |  1.9e-04 / 0.029  |
  1   64  600  1 |  2.1e-08 / 0.008  |  2.7e-06 / 0.029  |  3.3e-06 / 0.026  |

All of it is inside a quarter of the bounds (rstd: 2.4e-4, mean: 0.25).  The fp32 group fold is the larger part of the
offset(64) column: with group_fold="fp64" the four chunked 32-group rows read 3.5e-5, 4.3e-5, 4.7e-5 and 2.0e-5.  It grows as the
chunks get fewer -- (1, 240, 300, 24), three chunks, reads 6.1e-4, inside the bound but not a quarter of it, which is why the
one-lane-finalize row has 1000 pixels -- and with the fold's length: the single group of 64 channels (2048 terms) read 1.3e-3
in fp32, outside the rstd bound itself.  gn_partial_kernel therefore folds more than 128 terms in fp64; the models' 32 groups
give 64 to 80 terms and keep the fp32 fold, and with it their outputs bit for bit.
"""
import math

import numpy as np
import torch

from consistencytta_amd import spec

BF16_TOL = 1.5 * 2.0 ** -8          # the suite's constant (test_ops_gpu.py, test_bwd_ops_gpu.py)
GN_EPS = 1e-5
LN_EPS = 1e-5
SOFTMAX_FLOOR = 2.0 ** -120


def det(name, shape, seed=0):
    return torch.from_numpy(spec.det_uniform(name, tuple(shape), seed))


def bf16_round(x):
    return x.to(torch.bfloat16).to(torch.float32)


def f32(v):
    """The value a C float argument carries."""
    return float(np.float32(v))


def silu64(z):
    return z * torch.sigmoid(z)


def silu_grad64(z):
    s = torch.sigmoid(z)
    return s * (1.0 + z * (1.0 - s))


# ------------------------------------------------------------------------------------------------ references
def gn_forward_ref(x, G, gamma, beta, eps, silu):
    """x (B, hw, C) -> y (B, hw, C), mean (B, G), rstd (B, G), all float64; two-pass variance."""
    B, hw, C = x.shape
    cpg = C // G
    xs = x.double().view(B, hw, G, cpg)
    mean = xs.mean(dim=(1, 3))
    var = ((xs - mean.view(B, 1, G, 1)) ** 2).mean(dim=(1, 3))
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    z = (xs - mean.view(B, 1, G, 1)) * rstd.view(B, 1, G, 1) * gamma.double().view(G, cpg) + beta.double().view(G, cpg)
    y = silu64(z) if silu else z
    return y.reshape(B, hw, C), mean, rstd


def gn_apply_ref(x, G, gamma, beta, mean, rstd, silu):
    """The normalisation with GIVEN statistics (B, G), float64."""
    B, hw, C = x.shape
    cpg = C // G
    xs = x.double().view(B, hw, G, cpg)
    z = (xs - mean.double().view(B, 1, G, 1)) * rstd.double().view(B, 1, G, 1) * gamma.double().view(G, cpg) \
        + beta.double().view(G, cpg)
    return (silu64(z) if silu else z).reshape(B, hw, C)


def slab_max(t, G):
    """max|t| over each (sample, group) slab of a (B, hw, C) tensor, broadcast back to (B, hw, C)."""
    B, hw, C = t.shape
    m = t.abs().view(B, hw, G, C // G).amax(dim=(1, 3), keepdim=True)
    return m.expand(B, hw, G, C // G).reshape(B, hw, C)


def gn_backward_ref(x, dy, G, gamma, beta, eps, silu, stats=None):
    """Closed form of the GroupNorm(+SiLU) backward in float64.  stats (B, G, 2) = (mean, rstd): the statistics the kernel is
    handed (it never recomputes them); None: the exact ones.
      xhat = (x - mean) rstd, z = xhat gamma + beta, dz = dy silu'(z)
      dx = rstd (dz gamma - S1 / n - xhat S2 / n),  S1 = sum_slab dz gamma, S2 = sum_slab dz gamma xhat, n = hw C/G
      dgamma_c = sum_{b, pix} dz xhat,  dbeta_c = sum_{b, pix} dz
    Returns dx (B, hw, C), dgamma, dbeta, sum|dz xhat|, sum|dz| (the per-term absolute sums of param_bound)."""
    B, hw, C = x.shape
    cpg = C // G
    xs = x.double().view(B, hw, G, cpg)
    if stats is None:
        mean = xs.mean(dim=(1, 3))
        var = ((xs - mean.view(B, 1, G, 1)) ** 2).mean(dim=(1, 3))
        rstd = 1.0 / torch.sqrt(var + f32(eps))
    else:
        mean, rstd = stats.double()[..., 0], stats.double()[..., 1]
    mean, rstd = mean.view(B, 1, G, 1), rstd.view(B, 1, G, 1)
    gm, bt = gamma.double().view(G, cpg), beta.double().view(G, cpg)
    xhat = (xs - mean) * rstd
    dz = dy.double().view(B, hw, G, cpg)
    if silu:
        dz = dz * silu_grad64(xhat * gm + bt)
    n = hw * cpg
    s1 = (dz * gm).sum(dim=(1, 3), keepdim=True) / n
    s2 = (dz * gm * xhat).sum(dim=(1, 3), keepdim=True) / n
    dx = rstd * (dz * gm - s1 - xhat * s2)
    tg = dz * xhat
    return (dx.reshape(B, hw, C), tg.sum(dim=(0, 1)).reshape(C), dz.sum(dim=(0, 1)).reshape(C),
            tg.abs().sum(dim=(0, 1)).reshape(C), dz.abs().sum(dim=(0, 1)).reshape(C))


def ln_forward_ref(x, d, gamma, beta, eps):
    """x (rows, ld), columns >= d ignored -> y (rows, ld) float64 with zero pad columns."""
    xs = x.double()[:, :d]
    mean = xs.mean(dim=1, keepdim=True)
    var = ((xs - mean) ** 2).mean(dim=1, keepdim=True)
    y = torch.zeros(x.shape, dtype=torch.float64)
    y[:, :d] = (xs - mean) / torch.sqrt(var + f32(eps)) * gamma.double() + beta.double()
    return y


def ln_backward_ref(x, dy, d, gamma, eps):
    """Closed form of the LayerNorm backward in float64 (statistics recomputed, as the kernel does):
      dx = rstd (dy gamma - mean_c(dy gamma) - xhat mean_c(dy gamma xhat)),  dgamma_c = sum_r dy xhat,  dbeta_c = sum_r dy
    Returns dx (rows, ld) with zero pads, dgamma (d), dbeta (d), sum|dy xhat|, sum|dy|."""
    xs, ds = x.double()[:, :d], dy.double()[:, :d]
    mean = xs.mean(dim=1, keepdim=True)
    var = ((xs - mean) ** 2).mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    xhat = (xs - mean) * rstd
    dg = ds * gamma.double()
    dx = torch.zeros(x.shape, dtype=torch.float64)
    dx[:, :d] = rstd * (dg - dg.mean(dim=1, keepdim=True) - xhat * (dg * xhat).mean(dim=1, keepdim=True))
    tg = ds * xhat
    return dx, tg.sum(0), ds.sum(0), tg.abs().sum(0), ds.abs().sum(0)


def softmax_ref(s, cols, scale, bias=None, rows_per_bias=1):
    """s (rows, lds) fp32, columns >= cols ignored; bias (rows / rows_per_bias, cols) or None -> P (rows, cols) float64."""
    z = s.double()[:, :cols] * f32(scale)
    if bias is not None:
        z = z + bias.double().repeat_interleave(rows_per_bias, 0)[: z.shape[0]]
    z = z - z.amax(dim=1, keepdim=True)
    e = torch.exp(z)
    return e / e.sum(dim=1, keepdim=True)


def softmax_backward_ref(p, dp, cols, scale):
    """dS = P (dP - sum_j P_j dP_j) scale from the bf16 P the kernel is given.  Returns dS (rows, cols) and sum_j |P_j dP_j|."""
    pp, dd = p.double()[:, :cols], dp.double()[:, :cols]
    t = pp * dd
    return pp * (dd - t.sum(1, keepdim=True)) * f32(scale), t.abs().sum(1, keepdim=True)


# ------------------------------------------------------------------------------------------------ bounds
def fwd_bound(ref, M):
    """Forward, per element: |got - ref| <= 2^-8 |ref| + 2^-10 M.
    2^-8 |ref| is the bf16 round-to-nearest of the result: bf16 carries 8 significant bits, so half a unit in the last place is
    at most 2^-8 of the value, reached just above a power of two.  (It is ONCE that rounding, not twice: the fp32 evaluation
    has no room of its own in this term, only in the next -- which softmax does not have, so a softmax kernel passes only
    while its fp32 error stays orders of magnitude under 2^-8.  Measured: 0.99 of the bound from the rounding alone.)  2^-10 M, M the largest |ref| of the element's slab (GroupNorm)
    or row (LayerNorm), covers y = x scale + shift near a zero of y: there the two products are of size M and cancel, so the
    statistics' own error (relative 2^-10 for rstd at the worst, stats_bounds) stays of size 2^-10 M while |ref| -> 0.
    Softmax has no cancellation: M = 0."""
    return 2.0 ** -8 * ref.abs() + 2.0 ** -10 * M


def softmax_fwd_bound(ref):
    """Softmax forward, per element: |got - ref| <= 2^-8 |ref| + 2^-120 (fwd_bound with M = 0, plus a floor).  Under the floor
    `got` may be 0 or a denormal of a few bits: __expf flushes or truncates what falls under 2^-126, and the 1 / sum factor can
    push a result of up to 2^-120 there at the widths in use."""
    return 2.0 ** -8 * ref.abs() + SOFTMAX_FLOOR


def stats_bounds(mean_ref, rstd_ref):
    """stats_out: |mean - ref| <= 2^-20 (|ref| + std), |rstd - ref| <= 2^-10 ref  (std = 1 / rstd_ref).
    The mean is a sum of n values of size |mean| + std folded from fp32 partial sums: 2^-20 is 16 ulp of fp32.  The variance
    is E[x^2] - mean^2, which loses (mean / std)^2 of the partial sums' relative accuracy: at mean / std = 64 and partial
    sums good to 2^-23 that is 2^-11 on the variance, 2^-12 on rstd; 2^-10 leaves a factor four."""
    return 2.0 ** -20 * (mean_ref.abs() + 1.0 / rstd_ref), 2.0 ** -10 * rstd_ref


def emulation_bounds(mean_ref, rstd_ref):
    """stats_out against gn_stats_emulated: |mean - emulated| <= 2^-22 (|mean| + std), |rstd - emulated| <= 2^-22 rstd.
    The emulation adds the same fp32 numbers in the same order as the kernels up to the fp32 partial sums (bit for bit); what
    follows is fp64 in both, where another order moves the variance by 2^-40 at |mean| / std = 64; then each side rounds mean
    and rstd to fp32 once (2^-24).  Four times that rounding.  This is the summation CONTRACT (fp32 running sums per channel
    and chunk, the group fold of gn_group_fold, the chunks in fp64), far tighter than stats_bounds: folding the chunks in fp32 stays inside
    stats_bounds at the tables' shapes (measured 0.19 of it) and is fifty times outside this."""
    return 2.0 ** -22 * (mean_ref.abs() + 1.0 / rstd_ref), 2.0 ** -22 * rstd_ref


def slab_bound(ref_max):
    """dx / dS: max|got - ref| over a row or (sample, group) slab <= 2 * BF16_TOL * max|ref| over the same row or slab -- the
    bound test_bwd_ops_gpu.py uses per tensor, taken per row or slab."""
    return 2 * BF16_TOL * ref_max


def softmax_bwd_bound(ref, p, dot_abs, cols, scale):
    """Softmax backward, per element: 2^-8 |ref| + 2 cols 2^-24 scale p_c sum_j |p_j dp_j|.  The second term is the fp32 dot
    product's worst case (cols terms, each addition and product rounding once) carried through p_c (dp_c - dot) scale."""
    return 2.0 ** -8 * ref.abs() + 2.0 * cols * 2.0 ** -24 * f32(scale) * p.double() * dot_abs


def param_bound(n, abs_sum):
    """dgamma / dbeta per column: |got - ref| <= (n 2^-24 + 2^-20) sum|t|, n the number of terms t a column adds (rows for
    LayerNorm, B hw for GroupNorm), sum|t| their float64 absolute sum.  n 2^-24 sum|t| is the worst case of ANY fp32 summation
    order; 2^-20 sum|t| covers the fp32 xhat inside each term: (x - mean) rstd with mean good to 2^-24 |mean| is good to
    (|mean| / std) 2^-24, i.e. 2^-20 up to |mean| / std = 16 -- which is why the backward tables run offset(16) and leave
    offset(64) to the forward."""
    return (n * 2.0 ** -24 + 2.0 ** -20) * abs_sum


def worst_ratio(err, bound):
    """max err / bound; an element whose bound is 0 must be exact."""
    err = err.double()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    exact = torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err))
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), exact)
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ inputs
GN_KINDS = ("benign", "offset16", "offset64", "constant")
CONSTANT_VALUES = (0.5, 1.0, 1.5, 2.0)   # k * 0.5: every fp32 partial sum of them and of their squares is exact


def constant_slab(b, g):
    """Which (sample, group) slabs / rows the `constant` kind fills with one value."""
    return (b + g) % 2 == 0


def gn_input(kind, B, C, hw, G, tag):
    """(B, hw, C) fp32 holding bf16 values.
    benign: today's 0.3 +- 2 (|mean| / std = 0.26).  offsetR: +-(R / 4) +- 0.43, sign alternating by group; the uniform draw of every slab is
    standardised first, so that its mean is R / 4 and its std 0.43 / sqrt 3 whatever the slab's size: |mean| / std = R before
    the bf16 rounding, which moves it by well under a percent.  constant: benign, with every other slab one value of CONSTANT_VALUES (variance exactly 0)."""
    u = det("nf.gn.x." + tag, (B, hw, C), 1)
    cpg = C // G
    if kind in ("benign", "constant"):
        x = u * 2 + 0.3
        if kind == "constant":
            xv = x.view(B, hw, G, cpg)
            for b in range(B):
                for g in range(G):
                    if constant_slab(b, g):
                        xv[b, :, g, :] = CONSTANT_VALUES[(b + g // 2) % 4]
    else:
        ratio = {"offset16": 16.0, "offset64": 64.0}[kind]
        sign = torch.tensor([1.0 if g % 2 == 0 else -1.0 for g in range(G)]).view(1, 1, G, 1)
        uv = u.double().view(B, hw, G, cpg)
        uv = (uv - uv.mean(dim=(1, 3), keepdim=True)) / uv.var(dim=(1, 3), unbiased=False, keepdim=True).sqrt()
        x = (uv * (0.43 / math.sqrt(3.0)) + sign * (ratio / 4.0)).float().reshape(B, hw, C)
    return bf16_round(x).contiguous()


def rows_input(kind, rows, d, ld, tag, pad=7.0):
    """(rows, ld) fp32 holding bf16 values, the LayerNorm twin of gn_input (per row).  Columns >= d hold `pad`: the kernels
    must not let them into the statistics."""
    u = det("nf.ln.x." + tag, (rows, d), 1)
    if kind in ("benign", "constant"):
        x = u * 3 + 0.5
        if kind == "constant":
            for r in range(0, rows, 2):
                x[r, :] = CONSTANT_VALUES[(r // 2) % 4]
    else:
        ratio = {"offset16": 16.0, "offset64": 64.0}[kind]
        sign = torch.tensor([1.0 if r % 2 == 0 else -1.0 for r in range(rows)]).view(rows, 1)
        uv = u.double()
        uv = (uv - uv.mean(dim=1, keepdim=True)) / uv.var(dim=1, unbiased=False, keepdim=True).sqrt()
        x = (uv * (0.43 / math.sqrt(3.0)) + sign * (ratio / 4.0)).float()
    out = torch.full((rows, ld), float(pad))
    out[:, :d] = x
    return bf16_round(out).contiguous()


def affine(C, tag):
    """gamma = 1 +- 0.2, beta = +- 0.1, the suite's."""
    return (1 + 0.2 * det("nf.g." + tag, (C,), 2)).contiguous(), (0.1 * det("nf.b." + tag, (C,), 3)).contiguous()


SOFTMAX_KINDS = ("benign", "equal", "spike60", "span80")


def softmax_scores(kind, rows, cols, lds, scale, tag, pad=1.0e30):
    """fp32 scores (rows, lds); columns >= cols hold `pad` (a kernel that read them would show it).
    benign: +- 30, the suite's.  equal: every score of a row the same (a different value per row).  spike60: one score 60
    above the rest AFTER scaling.  span80: scaled scores spanning +- 80."""
    sc = f32(scale)
    u = det("nf.sm.s." + tag, (rows, cols), 1)
    if kind == "benign":
        s = u * 30
    elif kind == "equal":
        s = (torch.arange(rows, dtype=torch.float32).view(rows, 1) * 3.0 - 5.0).expand(rows, cols).clone()
    elif kind == "spike60":
        s = u * (2.0 / sc)
        for r in range(rows):
            c = (r * 37 + cols - 1) % cols
            s[r] = torch.minimum(s[r], s[r, c])       # nothing above the chosen column's own score ...
            s[r, c] = s[r, c] + 60.0 / sc             # ... which then stands 60 above after scaling
    elif kind == "span80":
        s = u * (80.0 / sc)
        s[:, 0], s[:, cols - 1] = -80.0 / sc, 80.0 / sc
    else:
        raise ValueError(kind)
    out = torch.full((rows, lds), float(pad))
    out[:, :cols] = s
    return out.contiguous()


def softmax_bias(kind, nb, cols):
    """(nb, cols) additive bias.  zero / mask_all: every key of the odd bias rows masked with -10000 / mask_but_one: all but one."""
    bias = torch.zeros(nb, cols)
    for b in range(nb):
        if kind == "mask_all" and b % 2 == 1:
            bias[b, :] = -10000.0
        elif kind == "mask_but_one" and b % 2 == 1:
            bias[b, :] = -10000.0
            bias[b, (b * 13 + 5) % cols] = 0.0
        elif kind == "mask_tail":
            bias[b, cols // 2 + b:] = -10000.0
    return bias


# ------------------------------------------------------------------------------------------------ the dispatchers, restated
def gn_small_ok(hw, c, groups):
    """norm_elem.hip: gn_small_ok."""
    cpg = c // groups
    return cpg % 8 == 0 and hw * cpg <= 16384 and groups <= 65535


def gn_geometry(hw, c):
    """norm_elem.hip: gn_geometry -> (pixels per chunk, chunks)."""
    ppc = max(16, min(1024, 32768 // c))
    ppc = min(ppc, hw)
    return ppc, (hw + ppc - 1) // ppc


def gn_finalize_lanes(G):
    """norm_elem.hip: gn_finalize_kernel's lanes per group."""
    return min(64, 256 // G) if (G <= 128 and 256 % G == 0) else 1


GN_FOLD_FP32_TERMS = 128   # norm_elem.hip: GN_FOLD_FP32_TERMS


def gn_group_fold(C, G):
    """norm_elem.hip: gn_partial_kernel's fold of a group's per-lane, per-channel sums -- one running sum over
    lanes * channels per group terms, fp32 up to GN_FOLD_FP32_TERMS of them, fp64 (rounded to the fp32 partial) beyond."""
    VC = C // 8
    PL = 256 // VC if VC <= 256 else 1
    return "fp32" if PL * (C // G) <= GN_FOLD_FP32_TERMS else "fp64"


GN_FWD_FORMS = {"small", "partial:VC<=256", "partial:VC>256", "fold:fp32", "fold:fp64", "finalize:one lane per group",
                "finalize:lanes share a group",
                "finalize_wide", "apply:fixed column", "apply:moving column"}


def gn_fwd_forms(B, C, hw, G):
    """norm_elem.hip: ctta_groupnorm_stats_out's launches (the `nchunk * groups > 2048` test included)."""
    if gn_small_ok(hw, C, G):
        return {"small"}
    _, nchunk = gn_geometry(hw, C)
    VC = C // 8
    forms = {"partial:VC<=256" if VC <= 256 else "partial:VC>256", "fold:" + gn_group_fold(C, G)}
    if nchunk * G > 2048:
        forms.add("finalize_wide")
    else:
        forms.add("finalize:one lane per group" if gn_finalize_lanes(G) == 1 else "finalize:lanes share a group")
    forms.add("apply:fixed column" if 256 % VC == 0 else "apply:moving column")
    return forms


GN_PARTIALS_FORMS = {"fused", "finalize+apply", "finalize_wide+apply"}


def gn_partials_form(C, G, nchunk, stats):
    """norm_elem.hip: ctta_groupnorm_from_partials."""
    if not stats and nchunk * G <= 2048 and C <= 4096:
        return "fused"
    return "finalize_wide+apply" if nchunk * G > 2048 else "finalize+apply"


LN_FWD_FORMS = {"fast<32,1,8>", "fast<64,1,8>", "fast<64,2,4>", "rows<32>", "rows<64>", "kernel<2>", "kernel<4>"}


def ln_fwd_form(ld):
    """norm_elem.hip: ctta_layernorm's ld ladder."""
    if ld in (256, 512, 1024):
        return {256: "fast<32,1,8>", 512: "fast<64,1,8>", 1024: "fast<64,2,4>"}[ld]
    if ld <= 256:
        return "rows<32>"
    if ld <= 512:
        return "rows<64>"
    return "kernel<2>" if ld <= 1024 else "kernel<4>"


def ln_fwd_rows_per_block(ld):
    return {"fast<32,1,8>": 64, "fast<64,1,8>": 32, "fast<64,2,4>": 16, "rows<32>": 32, "rows<64>": 16, "kernel<2>": 4,
            "kernel<4>": 4}[ln_fwd_form(ld)]


SOFTMAX_FORMS = {"generic", "reg<1>", "reg<2>", "reg<4>"}


def softmax_form(cols):
    """norm_elem.hip: ctta_softmax_rows."""
    return {1024: "reg<1>", 2048: "reg<2>", 4096: "reg<4>"}.get(cols, "generic")


def gn_bwd_small_ok(hw, c, groups):
    """backward.hip: gn_bwd_small_ok."""
    if c % groups:
        return False
    cpg = c // groups
    if cpg % 8 or cpg > 128:
        return False
    vpr = cpg // 8
    return 256 % vpr == 0 and hw * vpr <= 256 * 8


GN_BWD_FORMS = {"small<silu=0,acc=0>", "small<silu=0,acc=1>", "small<silu=1,acc=0>", "small<silu=1,acc=1>", "partial:VC<=256",
                "partial:VC>256", "fold_slices", "fold", "apply_cols", "apply", "param:set", "param:accumulate"}


def gn_bwd_forms(B, C, hw, G, silu, acc_dx, acc_param):
    """backward.hip: ctta_groupnorm_bwd's launches."""
    forms = {"param:accumulate" if acc_param else "param:set"}
    if gn_bwd_small_ok(hw, C, G):
        forms.add("small<silu=%d,acc=%d>" % (int(bool(silu)), int(bool(acc_dx))))
        return forms
    VC, cpg = C // 8, C // G
    forms.add("partial:VC<=256" if VC <= 256 else "partial:VC>256")
    gpb = 1 if cpg >= 64 else 64 // cpg
    forms.add("fold_slices" if cpg * gpb <= 1024 else "fold")
    forms.add("apply_cols" if VC <= 256 else "apply")
    return forms


def gn_bwd_apply_cols_threads(C):
    """backward.hip: the block size of gn_bwd_apply_cols_kernel."""
    VC = C // 8
    return 256 // VC * VC


def ln_bwd_rows_per_block(rows):
    """backward.hip: ln_bwd_rows_per_block."""
    rpb = rows // 2048
    return 8 if rpb < 8 else (64 if rpb > 64 else (rpb + 7) // 8 * 8)


def ln_bwd_scratch_floats(rows, ld):
    """backward.hip: ctta_layernorm_bwd_scratch_floats."""
    blocks = -(-rows // ln_bwd_rows_per_block(rows))
    floats = blocks * 2 * ld
    return floats + 32 * 2 * ld if (blocks >= 16 and floats * 4 <= (64 << 20)) else 0


LN_BWD_FORMS = {"ln_bwd<1,half>", "ln_bwd<1>", "ln_bwd<2>", "ln_bwd<4>", "one block", "table, sliced fold",
                "table, 32-way sliced fold", "atomics"}


def ln_bwd_forms(rows, ld, scratch):
    """backward.hip: ctta_layernorm_bwd_ws -> (forms, blocks, slices of the fold, dynamic LDS bytes)."""
    rpb = ln_bwd_rows_per_block(rows)
    if -(-rows // rpb) < 16:
        rpb = rows
    blocks = -(-rows // rpb)
    forms = {"ln_bwd<1,half>" if ld <= 256 else "ln_bwd<1>" if ld <= 512 else "ln_bwd<2>" if ld <= 1024 else "ln_bwd<4>"}
    smem = (8 if ld <= 256 else 4) * 2 * ld * 4
    n_slices = 0
    if blocks == 1:
        forms.add("one block")
    elif scratch and ln_bwd_scratch_floats(rows, ld):
        slices = 32 if blocks >= 32 * 8 else (blocks + 7) // 8
        rps = -(-blocks // slices)
        n_slices = -(-blocks // rps)
        forms.add("table, 32-way sliced fold" if slices == 32 else "table, sliced fold")
    else:
        forms.add("atomics")
    return forms, blocks, n_slices, smem


# ------------------------------------------------------------------------------------------------ case tables
# ctta_groupnorm / _stats_out: (B, C, hw, G, the form the row is there for)
GN_FWD_CASES = [
    (2, 256, 2048, 32, "small"),                              # every register slot used
    (2, 256, 2049, 32, "apply:fixed column"),                 # one pixel over: three launches
    (2, 40, 45, 8, "partial:VC<=256"),                        # cpg % 8 != 0: three launches
    (1, 320, 300, 32, "apply:moving column"),                 # 256 % VC != 0
    (1, 2560, 208, 32, "partial:VC>256"),
    (2, 2048, 1031, 32, "finalize_wide"),                     # 65 chunks, ragged last chunk
    (1, 192, 700, 24, "small"),                               # G does not divide 256; 5600 elements per slab: one launch
    (1, 240, 1000, 24, "finalize:one lane per group"),        # the same G with cpg % 8 != 0: three launches
    (1, 64, 600, 1, "fold:fp64"),                             # G = 1: 64 lanes share the group; a 2048-term group fold
]
# ctta_groupnorm_from_partials on ctta_concat_channels_gn's partials: (B, C1, C2, hw, G, stats, form)
GN_PARTIALS_CASES = [
    (2, 328, 312, 300, 32, False, "fused"),                   # a group straddles the two sources
    (2, 328, 312, 300, 32, True, "finalize+apply"),
    (2, 1024, 1024, 1031, 32, False, "finalize_wide+apply"),
]
# ctta_layernorm: (rows, d, ld, form)
LN_FWD_CASES = [
    (37, 96, 96, "rows<32>"), (35, 189, 192, "rows<32>"), (21, 384, 384, "rows<64>"), (18, 381, 384, "rows<64>"),
    (9, 768, 768, "kernel<2>"), (6, 2040, 2048, "kernel<4>"),
    (67, 255, 256, "fast<32,1,8>"), (35, 512, 512, "fast<64,1,8>"), (19, 1020, 1024, "fast<64,2,4>"),   # ragged last block
]
# ctta_softmax_rows: (rows, cols, form)
SOFTMAX_CASES = [(5, 4, "generic"), (7, 36, "generic"), (6, 1000, "generic"), (3, 5000, "generic"), (4, 1028, "generic"),
                 (5, 1024, "reg<1>"), (5, 2048, "reg<2>"), (5, 4096, "reg<4>")]
# ctta_groupnorm_bwd: (B, C, hw, G, silu, accumulate_dx, accumulate_param, stats from the forward's stats_out?, form)
GN_BWD_CASES = [
    (2, 256, 64, 32, 0, 0, 0, False, "small<silu=0,acc=0>"), (2, 256, 64, 32, 0, 1, 1, True, "small<silu=0,acc=1>"),
    (2, 256, 64, 32, 1, 0, 1, True, "small<silu=1,acc=0>"), (2, 256, 64, 32, 1, 1, 0, False, "small<silu=1,acc=1>"),
    (2, 320, 1024, 32, 1, 0, 0, True, "fold_slices"), (2, 320, 1024, 32, 0, 1, 1, False, "apply_cols"),
    (1, 2560, 208, 32, 1, 0, 1, False, "apply"), (1, 2560, 208, 32, 0, 1, 0, True, "partial:VC>256"),
    (2, 1032, 24, 1, 1, 0, 0, True, "fold"), (2, 1032, 24, 1, 0, 1, 1, False, "fold"),
    (2, 40, 45, 8, 1, 1, 1, True, "partial:VC<=256"), (2, 40, 45, 8, 0, 0, 0, False, "partial:VC<=256"),
]
# ctta_layernorm_bwd / _add / _ws: (rows, d, ld, forms)
LN_BWD_CASES = [
    (50, 381, 384, ("ln_bwd<1>", "one block")),
    (136, 384, 384, ("table, sliced fold", "atomics")),       # 17 blocks, three slices
    (2050, 96, 96, ("ln_bwd<1,half>", "table, 32-way sliced fold")),
    (40, 768, 768, ("ln_bwd<2>",)),
    (20, 1275, 1280, ("ln_bwd<4>",)),
    (12, 2040, 2048, ("ln_bwd<4>",)),                         # exactly 64 KB of dynamic LDS
]
# ctta_softmax_bias_rows + ctta_softmax_bwd_rows: (rows, cols, ldp, rows per bias row, lds, with bias)
SOFTMAX_BIAS_CASES = [(12, 300, 304, 4, 300, True), (6, 1030, 1032, 3, 1030, True), (8, 37, 40, 1, 37, True),
                      (12, 300, 304, 4, 320, True), (6, 1030, 1032, 3, 1030, False)]
SOFTMAX_BIAS_KINDS = ("mask_tail", "mask_all", "mask_but_one")


# ------------------------------------------------------------------------------------------------ statistics emulation
def _seq_sum32(a, axis):
    """Sequential fp32 sum along `axis` (np.add.accumulate adds one term at a time in the array's type)."""
    return np.take(np.add.accumulate(a.astype(np.float32), axis=axis, dtype=np.float32), -1, axis=axis)


def _gn_chunked_sums(x, G, group_fold=None):
    """(sum, sum of squares) per group of ONE sample (hw, C), float64, as gn_partial_kernel + gn_fold_chunks leave them."""
    hw, C = x.shape
    cpg, VC = C // G, C // 8
    ppc, nchunk = gn_geometry(hw, C)
    PL = 256 // VC if VC <= 256 else 1
    if group_fold is None:
        group_fold = gn_group_fold(C, G)
    s = np.zeros(G, np.float64)
    q = np.zeros(G, np.float64)
    for ch in range(nchunk):
        xs = x[ch * ppc: min(hw, (ch + 1) * ppc)].astype(np.float32)
        steps = -(-xs.shape[0] // PL)
        pad = np.zeros((steps * PL, C), np.float32)             # a pixel past the chunk adds + 0.0: the same sums
        pad[: xs.shape[0]] = xs
        pad = pad.reshape(steps, PL, C)                         # lane tp walks pixels tp, tp + PL, ... in order
        ssum = _seq_sum32(pad, 0)                               # [PL][C]
        ssq = _seq_sum32(pad * pad, 0)                          # bf16 squares are exact in fp32
        # the group's fold: l-major, then its channels, one running sum, rounded to the fp32 the partials table holds
        gs = ssum.reshape(PL, G, cpg).transpose(1, 0, 2).reshape(G, PL * cpg)
        gq = ssq.reshape(PL, G, cpg).transpose(1, 0, 2).reshape(G, PL * cpg)
        if group_fold == "fp64":
            s += gs.astype(np.float64).sum(1).astype(np.float32).astype(np.float64)
            q += gq.astype(np.float64).sum(1).astype(np.float32).astype(np.float64)
        else:
            s += _seq_sum32(gs, 1).astype(np.float64)
            q += _seq_sum32(gq, 1).astype(np.float64)
    return s, q


def _gn_small_sums(x, G):
    """The same for gn_small_kernel: per-thread fp32 sums of its <= 8 vectors, an fp32 xor butterfly per wave, fp64 over 4 waves."""
    hw, C = x.shape
    cpg = C // G
    lanes = np.arange(64)
    s = np.zeros(G, np.float64)
    q = np.zeros(G, np.float64)
    for g in range(G):
        v = x[:, g * cpg:(g + 1) * cpg].astype(np.float32).reshape(-1, 8)      # vector idx = pix * vpr + cv
        pad = np.zeros((8 * 256, 8), np.float32)
        pad[: v.shape[0]] = v
        per_thread = pad.reshape(8, 256, 8).transpose(1, 0, 2).reshape(256, 64)
        for arr, out in ((per_thread, s), (per_thread * per_thread, q)):
            t = _seq_sum32(arr, 1).reshape(4, 64)
            for o in (32, 16, 8, 4, 2, 1):
                t = (t + t[:, lanes ^ o]).astype(np.float32)
            w = t[:, 0].astype(np.float64)
            out[g] = (w[0] + w[1]) + (w[2] + w[3])
    return s, q


def gn_stats_emulated(x, G, eps=GN_EPS, form=None, group_fold=None):
    """fp32 emulation of GroupNorm's statistics on x (B, hw, C): per-channel fp32 running sums of x and x^2 over a chunk's
    pixels, a fold over the group's channels (group_fold "fp32": one fp32 running sum; "fp64": the same in double, rounded to
    the fp32 partial; None: whichever gn_partial_kernel takes, gn_group_fold), an fp64 fold over the chunks, chunking as gn_geometry (form
    "chunked"); or the single-launch kernel's sums (form "small"; None: whichever ctta_groupnorm takes).  Returns (mean, rstd),
    (B, G) fp32 as stats_out holds them.  It exists so that the CPU test can show that the bounds are reachable."""
    xn = x.numpy() if torch.is_tensor(x) else x
    B, hw, C = xn.shape
    if form is None:
        form = "small" if gn_small_ok(hw, C, G) else "chunked"
    mean = np.zeros((B, G), np.float32)
    rstd = np.zeros((B, G), np.float32)
    n = float(hw * (C // G))
    for b in range(B):
        s, q = _gn_small_sums(xn[b], G) if form == "small" else _gn_chunked_sums(xn[b], G, group_fold)
        m = s / n
        var = np.maximum(q / n - m * m, 0.0)
        mean[b] = m.astype(np.float32)
        rstd[b] = (1.0 / np.sqrt(var + float(np.float32(eps)))).astype(np.float32)
    return torch.from_numpy(mean), torch.from_numpy(rstd)
