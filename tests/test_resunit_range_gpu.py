"""The fused HiFi-GAN ResBlock kernels (csrc/resunit.hip) over every shape their predicates accept, against float64.

ctta_resunit_supported / ctta_reschain_supported decide where the vocoder takes the fused path, so each (C, k) row of
resunit_range.D_MAX runs here at d = 1, at its largest dilation and, at C = 512, on both sides of the tile switch; each with a
sequence shorter than its halo (B = 3) and one ragged against two tiles and the halo (B = 2).  The chained kernel runs at the
frontier of its accepted dilation triples (test_resunit_range_cpu.py).  Shapes one step outside, an aliased output and a
sequence one position past the 32-bit per-sample limit are refused before any launch; the longest accepted sequences run and
are checked in three windows.

Reference: CPU float64 F.conv1d on the same bf16 operands, rounded to bf16 where the kernels round -- leaky_relu(x) as it is
staged, the conv1 intermediate, and (chained) the residual stream after units 0 and 1.  Two bounds per output:
  * max-abs: rel_err <= 2 * BF16_TOL per unit, 3 * BF16_TOL per chain (as tests/test_ops_gpu.py);
  * rel-L2, derived from the output's own bf16 rounding.  The kernel returns bf16(y32) with y32 the fp32 result, y32 = ref + e
    (e: fp32 summation order, and the rare intermediate whose bf16 rounding falls the other way; measured well below 2^-12 of
    ||ref||).  Round-to-nearest moves each element by at most half an ulp, and an element whose rounding e tips the other way
    lands at most 2|e_i| further from ref_i than bf16(ref_i) does, so ||bf16(y32) - ref|| <= ||bf16(ref) - ref|| + 2||e||:
        rel_l2(out, ref) <= rel_l2(bf16(ref), ref) + 2^-11     (one unit; 2^-10 for three chained units)
    bf16(ref) - ref is the rounding error the kernel must make, about ulp / sqrt(12) per element (~1.5e-3 relative).
    Truncating instead of rounding doubles it (~3e-3), a dropped tap or a wrong halo row adds errors of O(1 / sqrt(k C)) to
    whole rows: each fails this bound while the max-abs check may still pass.
Output buffers are pre-filled with NaN (every row must be written) and followed by a whole tile of sentinel rows (nothing may
be written past the last sample, even by a tile that runs past the sequence end)."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import cases
from consistencytta_amd import _native as N
from consistencytta_amd import modules, spec
from gpu_util import DEV, bf16_round, det, pack_conv_weight, rel_err, rel_l2, sync
from oracle import nets as onets
from resunit_range import (ANY, D_MAX, RESCHAIN_TILE, TILE_SWITCH_512, ChainPredicate, frontier, frontier_picks, halo1,
                           reschain_accepted, reschain_halo, reschain_max_len, resunit_geom, resunit_max_len)

from test_engines_gpu import REL_L2, REL_MAX  # noqa: E402  (the vocoder's stated bounds)
from test_options_gpu import option  # noqa: E402,F401  (fixture: set an option, defaults restored afterwards)

pytestmark = pytest.mark.gpu

BF16_TOL = 1.5 * 2.0 ** -8
L2_SLACK_UNIT, L2_SLACK_CHAIN = 2.0 ** -11, 2.0 ** -10
SENTINEL = -12352.0                   # exactly representable in bf16
HUGE_D = 10 ** 6                      # k = 1: no halo whatever the dilation
STATS = {}                            # width -> [outputs checked, worst rel_err, worst rel-L2] (printed by _report)


def lib():
    return N.lib()


def _record(C, err, l2):
    s = STATS.setdefault(C, [0, 0.0, 0.0])
    s[0] += 1
    s[1], s[2] = max(s[1], err), max(s[2], l2)


def _check(C, got, ref, n_units, what):
    err, l2 = rel_err(got, ref), rel_l2(got, ref)
    bound = rel_l2(bf16_round(ref.float()), ref) + (L2_SLACK_UNIT if n_units == 1 else L2_SLACK_CHAIN)
    _record(C, err, l2)
    assert err <= (2 if n_units == 1 else 3) * BF16_TOL, (what, err)
    assert l2 <= bound, (what, l2, bound)


@functools.lru_cache(maxsize=None)
def unit_weights(C, k, tag="rr"):
    """bf16-rounded conv weights (CPU fp32) and their device copies: fragment-major weights, fp32 biases."""
    w1 = bf16_round(det("%s.w1.%d.%d" % (tag, C, k), (C, C, k), 2) * (1.0 / math.sqrt(C * k)))
    w2 = bf16_round(det("%s.w2.%d.%d" % (tag, C, k), (C, C, k), 3) * (1.0 / math.sqrt(C * k)))
    b1, b2 = det("%s.b1.%d.%d" % (tag, C, k), (C,), 4) * 0.1, det("%s.b2.%d.%d" % (tag, C, k), (C,), 5) * 0.1
    frags = []
    for w in (w1, w2):
        wp, k_pad = pack_conv_weight(w[:, :, None, :])
        f = torch.empty(C * k * C, dtype=torch.bfloat16, device=DEV)
        N.check(lib().ctta_frag_pack(N.ptr(wp), C, k_pad, k * C, N.ptr(f), N.stream_ptr()))
        frags.append(f)
    sync()
    return (w1, b1, w2, b2), (frags[0], b1.to(DEV), frags[1], b2.to(DEV))


def unit_ref(x, w, k, d):
    """float64 x + conv2(lrelu(conv1_d(lrelu(x)))) on (B, C, L) bf16 values, rounded where the kernel rounds."""
    w1, b1, w2, b2 = (t.double() for t in w)
    xa = bf16_round(F.leaky_relu(x.float(), 0.1)).double()            # the staged tile is bf16
    mid = F.leaky_relu(F.conv1d(xa, w1, b1, dilation=d, padding=d * (k - 1) // 2), 0.1)
    mid = bf16_round(mid.float()).double()                            # the intermediate is bf16 in LDS
    return x.double() + F.conv1d(mid, w2, b2, padding=(k - 1) // 2)


def chain_ref(x, ws, k, dils):
    r = x.double()
    for u, d in enumerate(dils):
        r = unit_ref(r, ws[u], k, d)
        if u < 2:
            r = bf16_round(r.float()).double()                        # the residual stream is bf16 between units
    return r


def device_x(x):
    return x.permute(0, 2, 1).contiguous().to(torch.bfloat16).to(DEV)


def guarded_out(n, spare, fill=float("nan")):
    """A flat bf16 buffer: n elements of `fill`, then `spare` sentinel elements."""
    out = torch.empty(n + spare, dtype=torch.bfloat16, device=DEV)
    out[:n].fill_(fill)
    out[n:].fill_(SENTINEL)
    return out


def check_guard(out, n, what):
    assert not bool(torch.isnan(out[:n]).any()), "%s: rows left unwritten" % what
    assert bool((out[n:] == SENTINEL).all()), "%s: written past the last sample" % what


def run_unit(x_d, B, L, C, k, d, wd, out, accumulate=0, alpha=1.0, out_slope=0.0):
    f1, b1, f2, b2 = wd
    N.check(lib().ctta_resunit_conv1d(N.ptr(x_d), B, L, C, k, d, N.ptr(f1), N.ptr(b1), N.ptr(f2), N.ptr(b2), 0.1, N.ptr(out),
                                      accumulate, alpha, out_slope, N.stream_ptr()))


def unit_dilations(C, k):
    d_max = D_MAX[(C, k)]
    ds = [1, HUGE_D] if d_max is ANY else [1, d_max]
    if C == 512:
        ds += [TILE_SWITCH_512[k] - 1, TILE_SWITCH_512[k]]
    return sorted(set(ds))


def extents(C, k, d):
    """(B, L): a sequence shorter than the conv1 halo (L = 1 when the halo is at most 2), and one ragged against two tiles."""
    h1, T = halo1(k, d), resunit_geom(C, k, d)[0]
    return [(3, 1 if h1 <= 2 else h1 - 1), (2, 2 * T + h1 + 5)]


UNIT_CASES = [(C, k, d, B, L) for (C, k) in sorted(D_MAX) for d in unit_dilations(C, k) for (B, L) in extents(C, k, d)]


@pytest.mark.parametrize("C,k,d,B,L", UNIT_CASES)
def test_resunit_accepted_shape_against_float64(C, k, d, B, L):
    assert lib().ctta_resunit_supported(C, k, d) == 1
    w, wd = unit_weights(C, k)
    x = bf16_round(det("rr.x.%d.%d.%d" % (C, k, L), (B, C, L), 1))
    xd = device_x(x)
    n, T = B * L * C, resunit_geom(C, k, d)[0]
    out = guarded_out(n, T * C)
    run_unit(xd, B, L, C, k, d, wd, out)
    sync()
    check_guard(out, n, (C, k, d, B, L))
    got = out[:n].view(B, L, C).permute(0, 2, 1).float().cpu()
    _check(C, got, unit_ref(x, w, k, d), 1, (C, k, d, B, L))


EPI_CASES = [(C, k, HUGE_D if D_MAX[(C, k)] is ANY else D_MAX[(C, k)]) for (C, k) in sorted(D_MAX)]


@pytest.mark.parametrize("C,k,d", EPI_CASES)
def test_resunit_stage_fold_epilogue_at_the_largest_dilation(C, k, d):
    """accumulate = 1, alpha = 1/3, out_slope = 0.01: out <- leaky_relu((out + unit) / 3, 0.01), the last ResBlock of a stage."""
    w, wd = unit_weights(C, k)
    T = resunit_geom(C, k, d)[0]
    B, L = 2, 2 * T + halo1(k, d) + 5
    x = bf16_round(det("rre.x.%d.%d" % (C, k), (B, C, L), 1))
    old = bf16_round(det("rre.o.%d.%d" % (C, k), (B, C, L), 6))
    n = B * L * C
    out = guarded_out(n, T * C)
    out[:n].copy_(device_x(old).reshape(-1))
    run_unit(device_x(x), B, L, C, k, d, wd, out, 1, 1.0 / 3.0, 0.01)
    sync()
    check_guard(out, n, (C, k, d))
    ref = F.leaky_relu((old.double() + unit_ref(x, w, k, d)) / 3.0, 0.01)
    _check(C, out[:n].view(B, L, C).permute(0, 2, 1).float().cpu(), ref, 1, ("epilogue", C, k, d))


@functools.lru_cache(maxsize=None)
def chain_picks(C, k):
    return frontier_picks(frontier(reschain_accepted(ChainPredicate(lib(), C, k))))


CHAIN_ROLES = ("largest d0", "largest d2", "balanced", "hifigan")


@pytest.mark.parametrize("role", range(4), ids=CHAIN_ROLES)
@pytest.mark.parametrize("C,k", [(32, 3), (32, 5), (32, 7), (64, 3), (64, 5), (64, 7)])
def test_reschain_frontier_against_three_units_and_float64(C, k, role):
    """Frontier triples of the accepted set (resunit_range.frontier_picks): bit-identical to three unit launches, and float64."""
    dils = chain_picks(C, k)[role]
    print("reschain C=%d k=%d %s: dilations %s" % (C, k, CHAIN_ROLES[role], dils))
    dil_arr = (ctypes.c_int * 3)(*dils)
    assert lib().ctta_reschain_supported(C, k, dil_arr) == 1
    T = RESCHAIN_TILE[C]
    B, L = 2, 2 * T + reschain_halo(k, dils) + 5
    ws, wds = [], []
    for u in range(3):
        w, wd = unit_weights(C, k, "rrc%d" % u)
        ws.append(w)
        wds.append(wd)
    x = bf16_round(det("rrc.x.%d.%d" % (C, k), (B, C, L), 1))
    xd = device_x(x)
    n = B * L * C
    vp = lambda i: (ctypes.c_void_p * 3)(*[N.ptr(wd[i]) for wd in wds])
    out = guarded_out(n, T * C)
    N.check(lib().ctta_reschain_conv1d(N.ptr(xd), B, L, C, k, dil_arr, vp(0), vp(1), vp(2), vp(3), 0.1, N.ptr(out), 0, 1.0, 0.0,
                                       N.stream_ptr()))
    sync()
    check_guard(out, n, ("chain", C, k, dils))
    cur = xd
    for u, d in enumerate(dils):
        nxt = torch.empty_like(xd)
        run_unit(cur, B, L, C, k, d, wds[u], nxt)
        cur = nxt
    sync()
    assert torch.equal(out[:n], cur.reshape(-1)), "chained launch differs from three unit launches"
    _check(C, out[:n].view(B, L, C).permute(0, 2, 1).float().cpu(), chain_ref(x, ws, k, dils), 3, ("chain", C, k, dils))


def test_refusals_before_any_launch():
    """Each refused call gets buffers sized for the extent it passes, so a missing guard would cost a wrong answer, never an
    access outside an allocation; the outputs must come back untouched (nothing was launched)."""
    B = 2
    for (C, k), d_max in sorted(D_MAX.items()):
        if d_max is ANY:
            continue
        _, wd = unit_weights(C, k)
        L = 2 * resunit_geom(C, k, d_max)[0] + 5
        xd = torch.zeros(B, L, C, dtype=torch.bfloat16, device=DEV)
        out = torch.full((B, L, C), SENTINEL, dtype=torch.bfloat16, device=DEV)
        assert lib().ctta_resunit_supported(C, k, d_max + 1) == 0
        with pytest.raises(RuntimeError, match="outside the fused kernel's range"):
            run_unit(xd, B, L, C, k, d_max + 1, wd, out)
        if C == 512 and k == 3:
            with pytest.raises(RuntimeError, match="may not alias the input"):
                run_unit(xd, B, L, C, k, 1, wd, xd)
        sync()
        assert bool((out == SENTINEL).all())
    _, wd = unit_weights(512, 5)
    xd = torch.zeros(B, 200, 512, dtype=torch.bfloat16, device=DEV)
    out = torch.empty_like(xd)
    assert lib().ctta_resunit_supported(512, 5, 1) == 0
    with pytest.raises(RuntimeError, match="outside the fused kernel's range"):
        run_unit(xd, B, 200, 512, 5, 1, wd, out)
    with pytest.raises(RuntimeError, match="may not alias the input"):
        run_unit(xd, B, 200, 64, 3, 1, unit_weights(64, 3)[1], xd)


def _window_check(x_d, out, L, C, lo, hi, margin, ref_fn, n_units, what):
    """Output positions [lo, hi) against a float64 reference computed from input positions [lo - margin, hi + margin) only
    (clipped to the sequence): the convolutions are local, and `margin` covers every halo."""
    a, b = max(0, lo - margin), min(L, hi + margin)
    xs = x_d[a * C:b * C].view(1, b - a, C).permute(0, 2, 1).float().cpu()
    ref = ref_fn(xs)[:, :, lo - a:hi - a]
    got = out[lo * C:hi * C].view(1, hi - lo, C).permute(0, 2, 1).float().cpu()
    _check(C, got, ref, n_units, (what, lo, hi))


def test_resunit_longest_accepted_sequence():
    """B = 1, C = 512, k = 3, d = 1 at the longest sequence the extent guard accepts (2^21 - 32 positions, 2 GiB per tensor):
    one position more is refused; the accepted run writes every row (no NaN left: reduced on the device), nothing past them,
    and its first, middle and last 300 positions match float64."""
    C, k, d = 512, 3, 1
    L = resunit_max_len(C, k, d)
    assert L == 2097120
    w, wd = unit_weights(C, k)
    n = (L + 1) * C                                   # sized for the refused extent: L + 1 positions
    x_d = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    x_d.uniform_(-1.0, 1.0, generator=torch.Generator(device=DEV).manual_seed(1234))
    out = guarded_out(L * C, C)
    with pytest.raises(RuntimeError, match="32-bit per-sample offsets"):
        run_unit(x_d, 1, L + 1, C, k, d, wd, out)
    run_unit(x_d, 1, L, C, k, d, wd, out)
    sync()
    check_guard(out, L * C, "resunit L=%d" % L)
    for lo in (0, L // 2 - 150, L - 300):
        _window_check(x_d, out, L, C, lo, lo + 300, 16, lambda xs: unit_ref(xs, w, k, d), 1, "resunit edge")
    del x_d, out
    torch.cuda.empty_cache()


def test_reschain_longest_accepted_sequence():
    """The chained kernel at C = 64, k = 3, (1, 3, 5) at its longest accepted sequence (2^24 positions, 2 GiB per tensor)."""
    C, k, dils = 64, 3, (1, 3, 5)
    L = reschain_max_len(C)
    assert L == 2 ** 24
    ws, wds = zip(*[unit_weights(C, k, "rrc%d" % u) for u in range(3)])
    n = (L + 1) * C
    x_d = torch.empty(n, dtype=torch.bfloat16, device=DEV)
    x_d.uniform_(-1.0, 1.0, generator=torch.Generator(device=DEV).manual_seed(4321))
    out = guarded_out(L * C, C)
    dil_arr = (ctypes.c_int * 3)(*dils)
    vp = lambda i: (ctypes.c_void_p * 3)(*[N.ptr(wd[i]) for wd in wds])
    run = lambda length: N.check(lib().ctta_reschain_conv1d(N.ptr(x_d), 1, length, C, k, dil_arr, vp(0), vp(1), vp(2), vp(3),
                                                            0.1, N.ptr(out), 0, 1.0, 0.0, N.stream_ptr()))
    with pytest.raises(RuntimeError, match="32-bit per-sample offsets"):
        run(L + 1)
    run(L)
    sync()
    check_guard(out, L * C, "reschain L=%d" % L)
    for lo in (0, L // 2 - 150, L - 300):
        _window_check(x_d, out, L, C, lo, lo + 300, reschain_halo(k, dils) + 8, lambda xs: chain_ref(xs, ws, k, dils), 3,
                      "reschain edge")
    del x_d, out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("fused", [1, 0])
def test_vocoder_with_dilations_8_and_10_at_512_channels(option, fused):
    """A full-width HiFi-GAN (first stage at 512 channels) whose k = 7 ResBlock has dilations (1, 8, 10): the fused path takes
    the 80-position tile there.  vocode against the oracle at the vocoder's REL_L2 / REL_MAX, and with "fused_res" = 0 (read
    when the handle is built) the conv_gemm path agrees within the same bounds without being bit-equal to the fused run."""
    hcfg = dict(spec.HIFIGAN_16K_64, upsample_initial_channel=1024, resblock_dilation_sizes=[[1, 3, 5], [1, 8, 10], [1, 3, 5]])
    assert all(lib().ctta_resunit_supported(512, 7, d) for d in (1, 8, 10)) and resunit_geom(512, 7, 8)[0] == 80
    sd = dict(cases.vae_weights(cases.TINY_VAE_DD))
    sd.update(cases.hifigan_weights(hcfg))
    mel = cases.mel_inputs(2, 12, 64, "rr_voc")

    def vocode():
        v = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=1.0, hifigan_config=hcfg)
        v.load_state_dict(sd)
        v.to(DEV).eval().requires_grad_(False)
        wav = v.vocode(mel.to(DEV)).float().cpu()
        del v
        return wav

    with torch.no_grad():
        ref = onets.hifigan_forward(hcfg, sd, mel.squeeze(1).permute(0, 2, 1)).squeeze(1)     # (B, 1, T) -> vocode's (B, T)
    wav = vocode()
    if fused == 0:
        option("fused_res", 0)
        wav_off = vocode()
        assert not torch.equal(wav_off, wav), "fused_res = 0 gave the fused run's bits: the fused path did not run"
        assert rel_l2(wav_off, wav) <= REL_L2 and rel_err(wav_off, wav) <= REL_MAX
        wav = wav_off
    assert wav.shape == ref.shape
    l2, mx = rel_l2(wav, ref), rel_err(wav, ref)
    print("vocoder (1, 8, 10) at 512 channels, fused_res=%d: rel_l2 %.3e, rel_max %.3e vs the oracle" % (fused, l2, mx))
    assert l2 <= REL_L2 and mx <= REL_MAX


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Cases run and the largest distances per width (printed with -s after the file's last test)."""
    yield
    for C in sorted(STATS):
        n, err, l2 = STATS[C]
        print("\nC=%4d: %3d outputs checked, max rel_err %.3e, max rel-L2 %.3e" % (C, n, err, l2), end="")
    print("\nunit (C, k, d, B, L) cases: %d; epilogue cases: %d" % (len(UNIT_CASES), len(EPI_CASES)))
