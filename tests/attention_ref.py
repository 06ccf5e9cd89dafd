"""CPU references for the flash-attention kernels, and the case lists their CPU and GPU tests share.

Two references of softmax(q k^T * scale + bias + rel) v on bf16-rounded q, k, v of shape (B, heads, n, dh):

  attention_fp64            the operation itself in float64, plus the log2-domain log-sum-exp the kernels hand to the backward;
  attention_bf16_emulated   the kernels' arithmetic: fp32 scores and exponentials in the log2 domain, P rounded to bf16 in front
                            of the PV product, normalised by the fp32 sum of the UNROUNDED P, output rounded to bf16.  It does not
                            model the tile-wise rescaling of the running maximum nor the hardware exp2.

`bias` is an additive per-key term (B, nk); `rel` is a relative-position table [heads][nq + nk - 1] indexed
key - query + nq - 1.  Both are in the natural-log domain (the kernels take the table pre-multiplied by log2 e).

The GPU tests bound each query row of the kernel's output by a multiple of what the emulation itself loses on that
case, so tests/test_attention_ref_cpu.py first pins the emulation inside half of the forward bound.
"""
import math

import torch

from consistencytta_amd import spec

LOG2E = 1.4426950408889634
BF16_TOL = 1.5 * 2.0 ** -8
ROW_BOUND = 2.5 * BF16_TOL          # the forward bound of test_attention, applied to every query row
KERNEL_OVER_EMULATION = 2.0         # tile-wise rescaling + v_exp_f32, which the emulation does not model

# (B, heads, dh, nq, nk, masked): test_attention's cases, then the routes no operator test entered (key tile = 64)
FWD_CASES_OLD = [(2, 3, 13, 256, 256, False), (2, 5, 51, 200, 200, False), (2, 6, 13, 4, 4, False),
                 (1, 2, 64, 130, 70, False), (2, 3, 13, 64, 7, True), (3, 5, 51, 300, 32, True)]
FWD_CASES_NEW = [(1, 2, 64, 130, 64, False),     # attention_kernel<3>, ragged nq
                 (2, 3, 40, 64, 64, False),      # attention_kernel<3>, whole tiles
                 (2, 2, 51, 130, 128, False),    # plain2 at its minimum, ragged nq
                 (2, 2, 51, 96, 192, False),     # plain2, three tiles (the tail tile_step)
                 (1, 2, 64, 160, 320, False)]    # plain2, five tiles, nq not a multiple of 128
FWD_CASES = FWD_CASES_OLD + FWD_CASES_NEW
# (B, heads, dh, nq, nk): ctta_attention_rel, always with ragged key masks
REL_CASES = [(3, 2, 64, 77, 77), (2, 3, 64, 150, 150), (2, 2, 64, 13, 13), (2, 2, 51, 130, 70)]
REL_ONE_OFFSET_CASE = (2, 2, 64, 77, 77)
REL_ONE_OFFSETS = (-3, 5)           # key - query of the only non-zero table entry, per head
REL_ONE_VALUE = 12.0
# (B, heads, dh, nq, nk, krows, use_bias): what test_flash_attention_backward gained
BWD_CASES_NEW = [(2, 2, 51, 64, 64, 64, False),       # PLAIN, one key tile
                 (1, 2, 64, 192, 192, 192, False),    # PLAIN, odd tile count
                 (1, 3, 40, 128, 320, 320, False),    # PLAIN, nq != nk
                 (2, 2, 51, 130, 128, 128, False)]    # plain2 forward with a non-plain backward


def det(name, shape, seed=0, scale=1.0):
    return torch.from_numpy(spec.det_uniform(name, shape, seed)) * scale


def bf16_round(x):
    return x.to(torch.bfloat16).to(torch.float32)


def ragged_key_bias(B, nk):
    """test_attention's masks: 0 for kept keys, -10000 behind each sample's length."""
    lens = [nk, max(1, nk // 2), max(1, nk - 3)][:B]
    keep = torch.arange(nk)[None, :] < torch.tensor(lens)[:, None]
    return (1 - keep.float()) * -10000.0


def fwd_inputs(B, heads, dh, nq, nk, masked, prefix="at"):
    """q, k, v, bias, scale exactly as test_attention draws them."""
    q = bf16_round(det(prefix + ".q", (B, heads, nq, dh), 1))
    k = bf16_round(det(prefix + ".k", (B, heads, nk, dh), 2))
    v = bf16_round(det(prefix + ".v", (B, heads, nk, dh), 3))
    return q, k, v, (ragged_key_bias(B, nk) if masked else None), 1.0 / math.sqrt(dh)


def rel_inputs(B, heads, dh, nq, nk, one_offset=False):
    """q, k, v, bias, rel table (natural-log domain), scale = 1 (T5 does not scale its scores)."""
    q, k, v, bias, _ = fwd_inputs(B, heads, dh, nq, nk, True, prefix="ar")
    if one_offset:
        rel = torch.zeros(heads, nq + nk - 1)
        for h in range(heads):
            rel[h, REL_ONE_OFFSETS[h % len(REL_ONE_OFFSETS)] + nq - 1] = REL_ONE_VALUE
    else:
        rel = det("ar.rel", (heads, nq + nk - 1), 4) * 2.0
    return q, k, v, bias, rel, 1.0


def _rel_term(rel, nq, nk):
    idx = torch.arange(nk)[None, :] - torch.arange(nq)[:, None] + nq - 1      # (nq, nk)
    return rel[:, idx]                                                       # (heads, nq, nk)


def attention_fp64(q, k, v, scale, bias=None, rel=None):
    """-> (out (B, heads, nq, dh) float64, lse2 (B, heads, nq) float64 = log2 sum_k exp(score))."""
    q, k, v = q.double(), k.double(), v.double()
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias.double()[:, None, None, :]
    if rel is not None:
        s = s + _rel_term(rel.double(), q.shape[2], k.shape[2])[None]
    lse = torch.logsumexp(s, dim=-1)
    out = torch.matmul(torch.exp(s - lse[..., None]), v)
    return out, lse * LOG2E


def f32_scalar(x):
    return float(torch.tensor(x, dtype=torch.float32))


def attention_bf16_emulated(q, k, v, scale, bias=None, rel=None):
    """-> out (B, heads, nq, dh) float32 holding bf16 values."""
    f32 = torch.float32
    q, k, v = q.to(f32), k.to(f32), v.to(f32)
    s = torch.matmul(q, k.transpose(-1, -2)) * f32_scalar(scale * LOG2E)
    if bias is not None:
        s = s + (bias.to(f32) * f32_scalar(LOG2E))[:, None, None, :]
    if rel is not None:
        s = s + _rel_term(rel.to(f32) * f32_scalar(LOG2E), q.shape[2], k.shape[2])[None]
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
    l = p.sum(dim=-1, keepdim=True)
    o = torch.matmul(bf16_round(p), v) / l
    return bf16_round(o)


def row_errors(got, ref):
    """Relative L2 error of every query row over its dh lanes: (B, heads, nq) float64."""
    got, ref = got.double(), ref.double()
    return (got - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)
