"""Host tables of the CLAP tower (`bicubic_taps`, `tap_tables`, `_window_perm`, `_merge_perm`, `_shift_mask`) and the
float64 references of tests/clap_ops_ref.py, on the CPU: the references against the oracle they restate, and the two
demonstrations the GPU bounds lean on (what a lost split pass costs, and how much of the log-mel gradient lives in the
halo samples)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clap_ops_ref as R
from consistencytta_amd import clap as C
from oracle import clap as oclap


# ------------------------------------------------------------------------------------------------ tap tables
@pytest.mark.parametrize("t_in,t_out", [(2, 64), (19, 64), (61, 64), (63, 64), (1001, 1024)])
def test_bicubic_taps_equal_interpolate(t_in, t_out):
    idx, w = C.bicubic_taps(t_in, t_out)
    assert idx.shape == (t_out, 4) and w.shape == (t_out, 4)
    assert int(idx.min()) >= 0 and int(idx.max()) < t_in
    assert float(np.abs(w.astype(np.float64).sum(1) - 1.0).max()) < 1e-6
    x = R.det64("taps.x.%d" % t_in, (3, t_in), 1)
    got = (x[:, torch.from_numpy(idx).long()] * torch.from_numpy(w).double()).sum(-1)
    ref = F.interpolate(x[:, None, :, None], (t_out, 1), mode="bicubic", align_corners=True)[:, 0, :, 0]
    # the taps are float32 (like torch's for float32 input).  The source position scale * i carries two float32
    # roundings of a value below t_in (t_in * 2^-23), the interpolant of samples in [-1, 1] has a slope below 3 per
    # sample, and each of the four weights is rounded once (2^-24 each): a wrong or shifted tap is off by O(0.1)
    err = float((got - ref).abs().max())
    print("t_in=%d: %.3e" % (t_in, err))
    assert err < 3 * t_in * 2.0 ** -23 + 4 * 2.0 ** -24


@pytest.mark.parametrize("t_in,t_out", [(2, 64), (19, 64), (63, 64), (64, 64), (150, 256), (256, 256)])
def test_tap_tables_csr_is_the_transpose(t_in, t_out):
    fe = C._FrontendState(dict(n_fft=1024, hop=480, mel_bins=64, sample_rate=48000, fmin=50, fmax=14000, spec_size=64,
                               patch_size=4))
    tabs = {k: v.numpy() for k, v in fe.tap_tables(t_in, t_out, "cpu").items()}
    idx, w = tabs["idx"].reshape(t_out, 4), tabs["w"].reshape(t_out, 4)
    fwd = np.zeros((t_out, t_in), np.float64)
    for tt in range(t_out):
        for k in range(4):
            fwd[tt, idx[tt, k]] += np.float64(w[tt, k])
    ptr, rt_tt, rt_w = tabs["rt_ptr"], tabs["rt_tt"], tabs["rt_w"]
    assert ptr.shape == (t_in + 1,) and ptr[0] == 0 and ptr[-1] == 4 * t_out == len(rt_tt) == len(rt_w)
    assert bool((np.diff(ptr) >= 0).all())
    bwd = np.zeros((t_out, t_in), np.float64)
    for t in range(t_in):
        for e in range(ptr[t], ptr[t + 1]):
            bwd[rt_tt[e], t] += np.float64(rt_w[e])
    # float64 sums of at most four float32 weights per cell, added in the same order by both forms
    assert bool((fwd == bwd).all())
    if t_in == t_out:
        assert bool((fwd == np.eye(t_out)).all())


# ------------------------------------------------------------------------------------------------ permutations
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("res,ws,shift", [(16, 8, 0), (16, 8, 4), (8, 8, 0), (4, 4, 0)])
def test_window_perm_matches_roll_and_partition(res, ws, shift, B):
    idx, inv = C._window_perm(B, res, ws, shift)
    n = B * res * res
    assert idx.dtype == torch.int32 and inv.dtype == torch.int32
    assert torch.equal(idx.long()[inv.long()], torch.arange(n)) and torch.equal(inv.long()[idx.long()], torch.arange(n))
    img = torch.arange(n).view(B, res, res, 1)
    if shift:
        img = torch.roll(img, (-shift, -shift), (1, 2))
    assert torch.equal(idx.long(), oclap.window_partition(img, ws).reshape(-1))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("res", [2, 4, 16])
def test_merge_perm_matches_patch_merging_concat(res, B):
    idx, inv = C._merge_perm(B, res)
    n = B * res * res
    assert torch.equal(idx.long()[inv.long()], torch.arange(n)) and torch.equal(inv.long()[idx.long()], torch.arange(n))
    x = torch.arange(n).view(B, res, res, 1)
    cat = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
    assert torch.equal(idx.long(), cat.reshape(-1))


@pytest.mark.parametrize("res,ws,shift", [(16, 8, 4), (8, 4, 2), (64, 8, 4)])
def test_shift_mask_equals_oracle(res, ws, shift):
    got, ref = C._shift_mask(res, res, ws, shift), oclap.shift_attn_mask(res, res, ws, shift)
    assert got.shape == ((res // ws) ** 2, ws * ws, ws * ws)
    assert torch.equal(got, ref)
    assert float(got.min()) == -100.0 and float(got[0].abs().max()) == 0.0      # window 0 never wraps


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("L", R.LOGMEL_LENGTHS)
def test_logmel_reference_agrees_with_the_oracle(L):
    wav = R.logmel_inputs(L)
    ref = R.logmel_db_ref(wav)
    orc = oclap.logmel(oclap.spectrogram_power(wav))[:, 0]
    assert ref.shape == orc.shape == (2, L // 480 + 1, 64)
    mel = R.mel_power64(wav, R.FRONT_CFG)
    # every mel value is exactly 0 (the -100 dB floor) or far above amin: no value where the clamp decides the answer
    assert not bool(((mel > 0) & (mel < 1e-6)).any())
    live = mel > 0
    assert bool((ref[~live] == -100.0).all()) and bool((orc[~live] == -100.0).all())
    # float32 STFT sums of 1024 terms and a float32 log10: a few float32 steps of the power, in dB
    err = float((ref - orc.double())[live].abs().max())
    print("L=%d  float32 oracle vs float64 reference: %.3e dB" % (L, err))
    assert err < 2e-4
    assert bool(R.silent_frames(wav).any()) == (L >= 2400)


@pytest.mark.parametrize("L", R.LOGMEL_LENGTHS)
def test_a_lost_split_pass_costs_more_than_the_forward_bound(L):
    """The six-product split in float64 reproduces the reference to far below the bound; without its smallest product it
    misses the bound, so the GPU test notices a lost pass."""
    wav = R.logmel_inputs(L)
    ref = R.logmel_db_ref(wav)
    live = R.mel_power64(wav, R.FRONT_CFG) > 0
    full, norms = R.logmel_db_split_emulated(wav)
    smallest = int(np.argmin(norms))
    assert smallest < 3                                              # one of the three third-order products
    lost, _ = R.logmel_db_split_emulated(wav, drop=smallest)
    e_full, e_lost = float((full - ref)[live].abs().max()), float((lost - ref)[live].abs().max())
    print("L=%d  six products %.3e dB, without pass %d %.3e dB (bound %.1e)" % (L, e_full, smallest, e_lost, R.LOGMEL_FWD_DB))
    assert e_full < R.LOGMEL_FWD_DB / 4
    assert e_lost > R.LOGMEL_FWD_DB


@pytest.mark.parametrize("L", R.LOGMEL_LENGTHS + (9000,))
def test_rounded_backward_reference_and_halo_share(L):
    """The rounded restatement differs from the plain float64 gradient by bf16-sized amounts only, and the halo samples
    hold the share of the gradient the GPU tests' restricted bounds are there for."""
    wav = R.logmel_inputs(L)
    dlm = R.det64("clapops.dlm.%d" % L, (2, L // 480 + 1, 64), 12)
    plain = R.logmel_db_bwd_ref(wav, dlm)
    rounded = R.logmel_db_bwd_rounded_ref(wav, dlm)
    rel = float((rounded - plain).abs().max() / plain.abs().max())
    halo = R.halo_mask(L)
    share = float((plain[:, halo] ** 2).sum() / (plain ** 2).sum())
    print("L=%d  rounded vs plain %.3e of max, halo share of |d wav|^2 %.1f %%" % (L, rel, 100 * share))
    # two bf16 roundings of 2^-9 each on every term of sums that partly cancel: a few 2^-9 of the largest element, not 0
    assert 2.0 ** -12 < rel < 2.0 ** -6
    assert share == 1.0 if L <= 1024 else 0.0 < share < 1.0
    # silent frames carry no gradient in either form
    sil = R.silent_frames(wav)
    if bool(sil.any()):
        dlm0 = dlm.clone()
        dlm0[sil] = 0.0
        assert torch.equal(R.logmel_db_bwd_rounded_ref(wav, dlm0), rounded)
        assert torch.equal(R.logmel_db_bwd_ref(wav, dlm0), plain)


@pytest.mark.parametrize("S,Fq,ps,frames", R.IMAGE_GEOMETRIES)
def test_image_reference_is_the_oracle_fold(S, Fq, ps, frames):
    lm, scale, shift = R.image_inputs(S, Fq, ps, frames)
    cfg = dict(R.FRONT_CFG, spec_size=S, mel_bins=Fq)
    # the oracle's own stretch and fold (float32) on the same affine input
    x = (lm * scale + shift)[:, None]
    ratio, tt = S // Fq, S * (S // Fq)
    if frames < tt:
        x = F.interpolate(x, (tt, Fq), mode="bicubic", align_corners=True)
    x = x.permute(0, 1, 3, 2).reshape(2, 1, Fq, ratio, tt // ratio).permute(0, 1, 3, 2, 4).reshape(2, Fq * ratio, tt // ratio)
    ref = R.image_ref(lm, scale, shift, S)
    assert ref.shape == (2, S, S)
    assert float((ref - x.double()).abs().max()) < 1e-5 * float(ref.abs().max())
    assert cfg["spec_size"] // cfg["mel_bins"] == ratio
    # the same stretch from the host's float32 taps: float32 tap positions (see test_bicubic_taps_equal_interpolate)
    taps = R.image_ref(lm, scale, shift, S, host_taps=True)
    assert float((taps - ref).abs().max()) < (3 * frames * 2.0 ** -23 + 4 * 2.0 ** -24) * float(ref.abs().max())
    # token layout round trip
    G = S // ps
    dtok = R.det64("img.tok", (2, G * G, 64), 5)
    dimg = R.tokens_to_image(dtok, S, ps)
    assert float(dimg[1, 5, 6]) == float(dtok[1, (5 // ps) * G + 6 // ps, (5 % ps) * ps + 6 % ps])


def test_attention_reference_lse_and_mask():
    heads, hd, n, nw, nbb = R.ATTN_CASES[-1]
    q, k, v, go, bias, dead = R.attention_inputs(heads, hd, n, nw, nbb)
    out, lse = R.window_attention_ref(q, k, v, bias, hd ** -0.5)
    s = (q @ k.transpose(-1, -2)) * hd ** -0.5 + bias[torch.arange(nw) % nbb]
    assert float((torch.exp2(s * C.LOG2E - lse[..., None]).sum(-1) - 1).abs().max()) < 1e-12
    dq, dk, dv = R.window_attention_bwd_ref(q, k, v, bias, hd ** -0.5, go)
    b, k0 = dead
    assert float(dk[b, :, k0:].abs().max()) < 1e-30 and float(dv[b, :, k0:].abs().max()) < 1e-30
    assert float(dk[b, :, :k0].abs().max()) > 1e-2


@pytest.mark.parametrize("orig,new,L", R.RESAMPLE_CASES)
def test_resample_reference_agrees_with_the_oracle(orig, new, L):
    x = R.det64("clapops.rs.x", (2, L), 1).to(torch.float32) * 0.8
    ref = oclap.resample(x, orig, new, **R.KAISER)
    r64 = R.resample64(x, orig, new, **R.KAISER)
    assert r64.shape == ref.shape and r64.dtype == torch.float64
    # float32 sums of a few hundred taps against the same taps summed in float64
    assert float((r64 - ref.double()).abs().max()) < 1e-5 * float(r64.abs().max())
