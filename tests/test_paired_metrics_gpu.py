"""The paired metrics of the evaluation suite on the HIP path (audioldm_eval/eval.py:137-179: `lsd`, `ssim_stft`, `psnr`, `ssim`):
ctta_ssim_mean, ctta_lsd, ctta_psnr_mse and the |STFT| at the DFT lengths 743 / 1486 against the float64 numpy restatement of
their published definitions (tests/paired_metrics_ref.py), and `EvaluationHelper(paired_metrics=True)` end to end on two
directories of .wav files.

Every bound below is a multiple of a figure measured on the CPU on the very inputs of the test: the distance between the
restatement evaluated in float32 and in float64 and, for what is fed by the split-bf16 STFT, the distance after moving the
restatement's magnitudes by the bound that GEMM is held to elsewhere (`perturbed`)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cases  # noqa: E402
import paired_metrics_ref as R  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402
from consistencytta_amd import audioldm_eval as E  # noqa: E402
from consistencytta_amd import spec  # noqa: E402
from gpu_util import DEV, sync  # noqa: E402

pytestmark = pytest.mark.gpu

# The split-bf16 front ends are held to 5e-3 in the natural-log domain (tests/test_engines_gpu.py, FRONTEND_MAX_ABS of
# tests/test_vggish_gpu.py): `perturbed` moves every magnitude by a factor exp(5e-3 u), u uniform in [-1, 1).
SPLIT_BF16_LOG_BOUND = 5e-3

# ctta_ssim_mean on exact fp32 images: the restatement in float32 (products and window means rounded to float32) differs from
# float64 by 3.8e-10 to 2.3e-6 over the cases below (smallest: the unrelated (101, 372) and (201, 744) magnitudes at R = 2,
# 3.8e-10; R = 1: 2.3e-8 at least).  Moments formed in fp64 agree to the rounding of the final mean (a second fp64 evaluation
# with the kernel's summation order: 3e-12 at most), so every case is held to 2.6 times the SMALLEST of those figures; fp32
# moments anywhere miss it in all but the two largest R = 2 cases.
SSIM_ABS = 1e-9
# ctta_lsd on exact fp32 magnitudes: float32 restatement against float64 1.6e-9 to 9.3e-7 (values 0.84 to 11.1); 2.5 times the
# smallest figure, for the same reason.
LSD_ABS = 4e-9
# Split-bf16 STFT against the float64 DFT sum, relative L2: the float32 restatement (float32 frames, tables and BLAS product)
# differs by 2.6e-7 to 2.7e-7 over whole spectrograms and by up to 3.5e-7 on the first / last frame alone; four times the
# larger figure.  (tests/test_ops_gpu.py holds the same entry point to 2e-6 at the loss's DFT lengths.)
STFT_REL_L2 = 1.4e-6
# ctta_psnr_mse on exact fp32 mels: a float32 mean of the squares differs from float64 by 6.9e-8 relative; twice that.
PSNR_MSE_REL = 1.4e-7
# EvaluationHelper against the restatement on the files of the end-to-end test.  float32 restatement against float64: lsd 8.4e-8,
# ssim_stft 5.4e-10, psnr 3.9e-7, ssim 5.7e-8.  Magnitudes moved by SPLIT_BF16_LOG_BOUND (`perturbed("e2e")`, each side of a pair
# on its own; psnr / ssim over the seven pairs that count, an identical pair stays identical on the HIP path): lsd 7.0e-6 (of
# 1.2069), ssim_stft 3.9e-6 (of 0.0674), psnr 1.3e-4 dB (of 21.078; 3.3e-5 to 1.3e-4 over three draws), ssim 1.3e-5 (of
# 0.4043).  Three times the larger figure of each key.
E2E_ABS = {"lsd": 2.1e-5, "ssim_stft": 1.2e-5, "psnr": 4.0e-4, "ssim": 3.9e-5}

SSIM_SHAPES = [(7, 7), (8, 9), (13, 64), (64, 101), (101, 372), (201, 744)]
_CACHE = {}


def perturbed(tag):
    """Every call of the returned function draws its own factors: the two sides of a pair move independently."""
    calls = []

    def f(mag):
        calls.append(0)
        u = spec.det_uniform("paired.perturb.%s.%d" % (tag, len(calls)), mag.shape, 7).astype(np.float64)
        return mag * np.exp(SPLIT_BF16_LOG_BOUND * u).astype(mag.dtype)
    return f


def spectra():
    """Two (201, 744) magnitude spectrograms of 2 s `eval_waves` clips (n_fft 1486, hop 320), scaled to the few hundred the
    peak-normalised audio of the LSD reaches; every image and spectrogram of the kernel tests is cut from them."""
    if "spectra" not in _CACHE:
        wav = cases.eval_waves("paired.img", 2, 64000, sr=32000).numpy().astype(np.float64)
        _CACHE["spectra"] = [(4.0 * R.stft_magnitude(w, 1486, 320)).astype(np.float32) for w in wav]
    return _CACHE["spectra"]


def rows_of(H, least):
    return [H, max(least, H - 3), max(least, H // 2)]


def ssim_case(H, W, data_range):
    """Three pairs of (H, W) fp32 images with rows_of(H, 7) valid rows: two unrelated images; an image against itself; two
    images whose left part is constant (variance exactly 0: S rests on C1 and C2 there).  data_range 2: magnitudes up to a few
    hundred; 1: their dB map clipped to [0, 1], like the normalised mel.  Rows past the valid ones hold NaN: they are not read."""
    key = ("ssim", H, W, data_range)
    if key not in _CACHE:
        a, b = (m[:H, :W].copy() for m in spectra())
        if data_range == 1.0:
            a, b = (np.clip((20 * np.log10(np.maximum(m, 1e-5)) + 50) / 100, 0, 1).astype(np.float32) for m in (a, b))
        k = max(7, W // 2)
        ac, bc = a.copy(), b.copy()
        ac[:, :k], bc[:, :k] = (0.75, 0.5) if data_range == 1.0 else (192.0, 128.0)     # sums of 49 squares are exact in fp64
        x, y, rows = np.stack([a, a, ac]), np.stack([b, a, bc]), rows_of(H, 7)
        ref = [R.ssim(x[p, :h], y[p, :h], data_range) for p, h in enumerate(rows)]
        ref32 = [R.ssim(x[p, :h], y[p, :h], data_range, dtype=np.float32) for p, h in enumerate(rows)]
        for p, h in enumerate(rows):
            x[p, h:], y[p, h:] = np.nan, np.nan
        _CACHE[key] = (x, y, rows, ref, ref32)
    return _CACHE[key]


def lsd_case(frames, bins):
    """Three pairs of (frames, bins) magnitudes with rows_of(frames, 1) valid frames: two unrelated spectrograms; a spectrogram
    against a quarter of itself (LSD = 2 log10 4); a generated spectrogram with exact zeros in it."""
    key = ("lsd", frames, bins)
    if key not in _CACHE:
        a, b = (m[:frames, :bins].copy() for m in spectra())
        z = a.copy()
        z[::3, ::5] = 0.0
        est, tgt, rows = np.stack([a, a, z]), np.stack([b, (0.25 * a).astype(np.float32), b]), rows_of(frames, 1)
        ref = [R.lsd(est[p, :h], tgt[p, :h]) for p, h in enumerate(rows)]
        ref32 = [R.lsd(est[p, :h], tgt[p, :h], dtype=np.float32) for p, h in enumerate(rows)]
        for p, h in enumerate(rows):
            est[p, h:], tgt[p, h:] = np.nan, np.nan
        _CACHE[key] = (est, tgt, rows, ref, ref32)
    return _CACHE[key]


def stft_case(n_fft, seconds, pad_mode, amp):
    key = ("stft", n_fft, seconds, pad_mode, amp)
    if key not in _CACHE:
        sr = {743: 16000, 1486: 32000}[n_fft]
        wav = (cases.eval_waves("paired.stft", 2, seconds * sr, sr=sr) * amp).contiguous()
        ref = np.stack([R.stft_magnitude(w.astype(np.float64), n_fft, R.hop_of(sr), pad_mode) for w in wav.numpy()])
        ref32 = np.stack([R.stft_magnitude(w, n_fft, R.hop_of(sr), pad_mode, dtype=np.float32) for w in wav.numpy()])
        _CACHE[key] = (wav, R.hop_of(sr), ref, ref32)
    return _CACHE[key]


def mel_pair():
    """The normalised mels (float32, (64, 201)) of two 2 s `eval_waves` clips, as the restatement computes them."""
    if "mels" not in _CACHE:
        wav = cases.eval_waves("paired.mel", 2, 32000).numpy()
        _CACHE["mels"] = [R.normalised_mel(w, 16000).astype(np.float32) for w in wav]
    return _CACHE["mels"]


def lengths(v):
    return (N.c_int32 * len(v))(*v)


def run_ssim(x, y, rows, data_range, win=7):
    P, H, W = x.shape
    L_ = N.lib()
    x_d, y_d = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    out = torch.full((P,), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.empty(P * max(1, L_.ctta_ssim_tiles(H, W, win)), dtype=torch.float64, device=DEV)
    N.check(L_.ctta_ssim_mean(N.ptr(x_d), N.ptr(y_d), P, H, W, lengths(rows), win, data_range, 1, N.ptr(out), N.ptr(ws),
                              N.stream_ptr()))
    sync()
    return out.cpu().numpy()


def run_lsd(est, tgt, rows):
    P, F, B = est.shape
    e_d, t_d = torch.from_numpy(est).to(DEV), torch.from_numpy(tgt).to(DEV)
    out = torch.full((P,), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.empty(P * F, dtype=torch.float64, device=DEV)
    N.check(N.lib().ctta_lsd(N.ptr(e_d), N.ptr(t_d), P, F, B, lengths(rows), N.ptr(out), N.ptr(ws), N.stream_ptr()))
    sync()
    return out.cpu().numpy()


def run_mse(x, y, rows):
    P, H, W = x.shape
    x_d, y_d = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    out = torch.full((P,), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.empty(P * H, dtype=torch.float64, device=DEV)
    N.check(N.lib().ctta_psnr_mse(N.ptr(x_d), N.ptr(y_d), P, H, W, lengths(rows), N.ptr(out), N.ptr(ws), N.stream_ptr()))
    sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("data_range", [1.0, 2.0])
@pytest.mark.parametrize("H,W", SSIM_SHAPES)
def test_ssim_mean_matches_the_restatement(H, W, data_range):
    """ctta_ssim_mean on three pairs with different valid heights: one window (7, 7), sizes off the 24 x 32 tile, the mel shape,
    rows wider than a tile; the pair of identical images scores exactly 1."""
    x, y, rows, ref, ref32 = ssim_case(H, W, data_range)
    got = run_ssim(x, y, rows, data_range)
    for p in range(3):
        print("ssim (%d, %d) R=%g pair %d rows %d: HIP %.15f, float64 %.15f, |diff| %.3e (float32 restatement: %.3e)"
              % (H, W, data_range, p, rows[p], got[p], ref[p], abs(got[p] - ref[p]), abs(ref32[p] - ref[p])))
    assert got[1] == 1.0 and ref[1] == 1.0
    for p in (0, 2):
        assert abs(got[p] - ref[p]) <= SSIM_ABS, (H, W, data_range, p)
    assert np.array_equal(run_ssim(x, y, rows, data_range), got)         # fixed summation order: the same bits


def test_ssim_mean_refuses_images_smaller_than_a_window():
    x = np.zeros((2, 9, 9), np.float32)
    for H, W, rows in ((6, 9, [6, 6]), (9, 6, [9, 9]), (9, 9, [9, 6]), (9, 9, [10, 9])):
        with pytest.raises(RuntimeError):
            run_ssim(x[:, :H, :W].copy(), x[:, :H, :W].copy(), rows, 1.0)
    with pytest.raises(RuntimeError):
        run_ssim(x, x, [9, 9], 1.0, win=8)                               # an even window
    with pytest.raises(RuntimeError):
        run_ssim(x, x, [9, 9], 0.0)
    assert np.array_equal(run_ssim(x, x, [9, 9], 1.0), [1.0, 1.0])


@pytest.mark.parametrize("bins", [372, 744])
@pytest.mark.parametrize("frames", [1, 7, 101])
def test_lsd_matches_the_restatement(frames, bins):
    """ctta_lsd on three pairs with different valid frame counts; the scaled copy gives |2 log10 c|; exact zeros on the generated
    side run into the 1e-12 guards (log10 of about 1e28 there); two calls give identical bits."""
    est, tgt, rows, ref, ref32 = lsd_case(frames, bins)
    got = run_lsd(est, tgt, rows)
    for p in range(3):
        print("lsd (%d, %d) pair %d frames %d: HIP %.12f, float64 %.12f, |diff| %.3e (float32 restatement: %.3e)"
              % (frames, bins, p, rows[p], got[p], ref[p], abs(got[p] - ref[p]), abs(ref32[p] - ref[p])))
    assert float(est[2, 0, 0]) == 0.0 and ref[2] > ref[0]
    assert abs(got[1] - 2 * np.log10(4.0)) <= 1e-9
    for p in range(3):
        assert abs(got[p] - ref[p]) <= LSD_ABS, (frames, bins, p)
    assert np.array_equal(run_lsd(est, tgt, rows), got)


def test_lsd_refuses_a_pair_without_frames():
    a = np.ones((2, 4, 372), np.float32)
    for rows in ([4, 0], [5, 4]):
        with pytest.raises(RuntimeError):
            run_lsd(a, a, rows)
    with pytest.raises(RuntimeError):
        run_lsd(np.ones((257, 1, 8), np.float32), np.ones((257, 1, 8), np.float32), [1] * 257)    # more than CTTA_PAIR_MAX


def run_stft(n_fft, hop, pad_mode, wav):
    B, L = wav.shape
    L_ = N.lib()
    h = N.c_void_p()
    N.check(L_.ctta_stft_create_dft(n_fft, hop, int(pad_mode == "constant"), B, L, h))
    try:
        assert L_.ctta_stft_frames(h, L) == L // hop + 1
        out = torch.full((B, L // hop + 1, n_fft // 2 + 1), float("nan"), dtype=torch.float32, device=DEV)
        N.check(L_.ctta_stft_magnitude(h, N.ptr(wav.to(DEV)), B, L, N.ptr(out), N.stream_ptr()))
        sync()
        with pytest.raises(RuntimeError):                                # no backward on such a handle
            N.check(L_.ctta_stft_magnitude_bwd(h, N.ptr(out), B, L, N.ptr(out), N.stream_ptr()))
        with pytest.raises(RuntimeError):                                # shorter than the centre padding reflects
            N.check(L_.ctta_stft_magnitude(h, N.ptr(out), B, n_fft // 2, N.ptr(out), N.stream_ptr()))
    finally:
        L_.ctta_stft_destroy(h)
    return out.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("amp", [1.0, 1e-3])
@pytest.mark.parametrize("pad_mode", ["reflect", "constant"])
@pytest.mark.parametrize("n_fft,seconds", [(743, 1), (743, 2), (1486, 1), (1486, 2)])
def test_dft_stft_matches_the_float64_definition(n_fft, seconds, pad_mode, amp):
    """ctta_stft_create_dft + ctta_stft_magnitude at the odd length 743 (K padded to 768) and at 1486 (1536) against the DFT
    sum in float64: two clips, both paddings, full scale and -60 dB; the first and the last frame, which hold the padding, on
    their own."""
    wav, hop, ref, ref32 = stft_case(n_fft, seconds, pad_mode, amp)
    got = run_stft(n_fft, hop, pad_mode, wav)
    assert got.shape == ref.shape == (2, seconds * 100 + 1, n_fft // 2 + 1) and np.isfinite(got).all()
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    err, edge = rel(got, ref), max(rel(got[:, 0], ref[:, 0]), rel(got[:, -1], ref[:, -1]))
    print("stft n=%d %d s %s amp=%g: rel_l2 %.3e, edge frames %.3e (float32 restatement: %.3e)"
          % (n_fft, seconds, pad_mode, amp, err, edge, rel(ref32, ref)))
    assert err <= STFT_REL_L2 and edge <= STFT_REL_L2


def test_dft_stft_on_a_ten_second_clip():
    """1001 frames at n = 743: past the GEMM's largest row tile, and a row count that is no multiple of any."""
    wav = cases.eval_waves("paired.stft10", 1, 160000)
    ref = R.stft_magnitude(wav[0].numpy().astype(np.float64), 743, 160)[None]
    got = run_stft(743, 160, "reflect", wav)
    err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print("stft n=743 10 s: rel_l2 %.3e" % err)
    assert got.shape == (1, 1001, 372) and err <= STFT_REL_L2


def test_dft_stft_create_keeps_the_old_entry_strict():
    L_ = N.lib()
    h = N.c_void_p()
    with pytest.raises(RuntimeError):
        N.check(L_.ctta_stft_create(743, 160, 743, 1, 16000, h))         # fft_size % 64 != 0 stays refused there
    for bad in ((8, 160, 0), (743, 0, 0), (743, 160, 2)):
        with pytest.raises(RuntimeError):
            N.check(L_.ctta_stft_create_dft(bad[0], bad[1], bad[2], 1, 16000, h))


def test_psnr_mse_is_exactly_zero_for_identical_mels():
    """ctta_psnr_mse on (frames, 64) mels: a mel against itself (exactly 0: the pair the helper leaves out), against the other
    clip's and against a copy shifted by one frame, with different valid frame counts."""
    m = [np.ascontiguousarray(v.T) for v in mel_pair()]                  # (201, 64)
    shifted = np.roll(m[0], 1, axis=0)
    x, y, rows = np.stack([m[0], m[0], m[0]]), np.stack([m[0], m[1], shifted]), [201, 150, 101]
    ref = [R.mse(x[p, :h], y[p, :h]) for p, h in enumerate(rows)]
    for p, h in enumerate(rows):
        x[p, h:], y[p, h:] = np.nan, np.nan
    got = run_mse(x, y, rows)
    print("mse: HIP %s, float64 %s" % (got, ref))
    assert got[0] == 0.0 and ref[0] == 0.0 and np.isinf(R.psnr(m[0], m[0]))
    for p in (1, 2):
        assert ref[p] > 1e-4 and abs(got[p] - ref[p]) <= PSNR_MSE_REL * ref[p]
        assert abs(10 * np.log10(1.0 / got[p]) - R.psnr(x[p, :rows[p]], y[p, :rows[p]])) <= 1e-9
    assert np.array_equal(run_mse(x, y, rows), got)
    with pytest.raises(RuntimeError):
        run_mse(x, y, [201, 0, 101])


def e2e_files(root):
    """Eight pairs of 2 s clips, 16 kHz generated and 48 kHz ground truth; pair 3 holds the same audio on both sides (every
    generated sample three times: striding by 3 gives it back)."""
    from scipy.io import wavfile
    gen_dir, gt_dir = os.path.join(root, "gen"), os.path.join(root, "gt")
    os.mkdir(gen_dir)
    os.mkdir(gt_dir)
    n = 8
    gen = (cases.eval_waves("paired.e2e.gen", n, 32000).numpy() * 32767).astype(np.int16)
    gt = (cases.eval_waves("paired.e2e.gt", n, 96000, sr=48000).numpy() * 32767).astype(np.int16)
    names = ["clip_%02d.wav" % i for i in range(n)]
    for i, f in enumerate(names):
        wavfile.write(os.path.join(gen_dir, f), 16000, gen[i])
        wavfile.write(os.path.join(gt_dir, f), 48000, np.repeat(gen[i], 3) if i == 3 else gt[i])
    return gen_dir, gt_dir, names


def e2e_reference(gen_dir, gt_dir, names, **kw):
    pairs = [(E.read_centered_wav(os.path.join(gen_dir, f), 16000), E.read_centered_wav(os.path.join(gt_dir, f), 16000))
             for f in names]
    return R.paired_metrics(pairs, 16000, **kw)


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def test_evaluation_helper_fills_the_four_paired_keys(golden, tmp_path):
    """EvaluationHelper(paired_metrics=True).main against the restatement on the same files; the identical pair is left out
    of psnr / ssim and counted in lsd / ssim_stft; every other key as the plain helper reports it, which keeps the four NaN."""
    g = golden("eval_suite")
    cnn14 = E.Cnn14(features_list=["2048", "logits"]).to(DEV)
    cnn14.load_state_dict(cases.cnn14_weights(g["cnn14_keys"], g["cnn14_shapes"]), strict=True)
    gen_dir, gt_dir, names = e2e_files(str(tmp_path))
    helper = E.EvaluationHelper(16000, DEV, mel_model=cnn14, paired_metrics=True)
    res = helper.main(None, gen_dir, gt_dir)
    assert list(res) == E.EvaluationHelper.KEYS
    ref = e2e_reference(gen_dir, gt_dir, names)
    without = e2e_reference(gen_dir, gt_dir, [f for f in names if f != "clip_03.wav"])
    for k in E2E_ABS:
        print("%s: HIP %.4f, float64 restatement %.6f (without the identical pair %.6f)" % (k, res[k], ref[k], without[k]))
        assert np.isfinite(res[k]) and abs(res[k] - ref[k]) <= E2E_ABS[k] + 5e-5, k       # 5e-5: the helper rounds to 4 digits
    # the restatement skips the identical pair in psnr / ssim by itself; in lsd / ssim_stft its share is far above the bound
    assert ref["psnr"] == without["psnr"] and ref["ssim"] == without["ssim"]
    assert abs(ref["lsd"] - without["lsd"]) > 10 * E2E_ABS["lsd"] and abs(res["lsd"] - without["lsd"]) > 10 * E2E_ABS["lsd"]
    assert abs(res["ssim_stft"] - without["ssim_stft"]) > 10 * E2E_ABS["ssim_stft"]
    ds = E.MelPairedDataset(gen_dir, gt_dir, helper.mel_stft(), 16000)
    assert len(ds) == 8 and [ds.name(i) for i in range(8)] == names
    unskipped = helper.calculate_psnr_ssim([ds[i] for i in range(8) if i != 3])           # tuples, as a DataLoader hands them over
    assert abs(unskipped["psnr"] - ref["psnr"]) <= E2E_ABS["psnr"] and abs(unskipped["ssim"] - ref["ssim"]) <= E2E_ABS["ssim"]
    mel_gen, mel_gt, name, (a_gen, a_gt) = ds[3]
    assert name == "clip_03.wav" and mel_gen.shape == (64, 201) and mel_gen.dtype == np.float32
    assert np.array_equal(mel_gen, mel_gt) and np.array_equal(a_gen, a_gt) and a_gen.shape == (32000,)
    plain = E.EvaluationHelper(16000, DEV, mel_model=cnn14).main(None, gen_dir, gt_dir)
    for k in E.EvaluationHelper.KEYS:
        if k in E2E_ABS:
            assert np.isnan(plain[k]), k
        else:
            assert _same(res[k], plain[k]), (k, res[k], plain[k])
    # the other padding of the spectrogram is a different number, computed as well
    const = E.EvaluationHelper(16000, DEV, mel_model=cnn14, paired_metrics=True, stft_pad_mode="constant")
    got_c, ref_c = const.calculate_lsd(ds), e2e_reference(gen_dir, gt_dir, names, pad_mode="constant")
    assert abs(got_c["lsd"] - ref_c["lsd"]) <= E2E_ABS["lsd"] and abs(got_c["ssim_stft"] - ref_c["ssim_stft"]) <= E2E_ABS["ssim_stft"]
    assert abs(ref_c["lsd"] - ref["lsd"]) > 0.0
    # unpaired directories: -1, like the reference
    unpaired = helper.calculate_metrics(None, gen_dir, gt_dir, same_name=False)
    for k in E2E_ABS:
        assert unpaired[k] == -1, k


def test_evaluation_helper_refuses_clips_too_short_to_pair(golden, tmp_path):
    from scipy.io import wavfile
    g = golden("eval_suite")
    cnn14 = E.Cnn14(features_list=["2048", "logits"]).to(DEV)
    cnn14.load_state_dict(cases.cnn14_weights(g["cnn14_keys"], g["cnn14_shapes"]), strict=True)
    gen_dir, gt_dir = tmp_path / "gen", tmp_path / "gt"
    gen_dir.mkdir()
    gt_dir.mkdir()
    wav = (cases.eval_waves("paired.short", 2, 32000).numpy() * 32767).astype(np.int16)
    for i, n in enumerate((32000, 1000)):                                # the second generated file: 1000 samples
        wavfile.write(str(gen_dir / ("clip_%d.wav" % i)), 16000, wav[i, :n])
        wavfile.write(str(gt_dir / ("clip_%d.wav" % i)), 16000, wav[i])
    helper = E.EvaluationHelper(16000, DEV, mel_model=cnn14, paired_metrics=True)
    with pytest.raises(ValueError, match="time offset"):
        helper.main(None, str(gen_dir), str(gt_dir))
    ds = E.MelPairedDataset(str(gen_dir), str(gt_dir), None, 16000)
    with pytest.raises(ValueError, match="window"):
        helper.calculate_lsd(ds, time_offset=200)                        # 800 samples: 6 frames, no 7 x 7 window
