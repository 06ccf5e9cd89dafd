"""Frechet Audio Distance on the HIP path (audioldm_eval/metrics/fad.py): the 2x2 max-pooling against torch, the VGGish front
end against its float64 numpy definition, the embeddings against the fp32 torch restatement (tests/vggish_torch.py) and
`EvaluationHelper` end to end on two directories of .wav files."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cases  # noqa: E402
import vggish_torch as VT  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402
from consistencytta_amd import audioldm_eval as E  # noqa: E402
from gpu_util import DEV, bf16_round, det, rel_l2, sync  # noqa: E402

pytestmark = pytest.mark.gpu

# Split-bf16 STFT (three parts per operand, six products, fp32 accumulation) against float64, in the log domain: the bound the
# same machinery is held to in tests/test_engines_gpu.py, easier here since the offset 0.01 is a thousand times that path's
# clamp.  A float32 evaluation of the formula differs from float64 by 5e-6 to 9e-6 on these inputs; a figure far above 1e-4 would
# point to a real defect (window placement, DC row, mel edges) even below the bound.
FRONTEND_MAX_ABS = 5e-3
# bf16 weights and inter-layer activations (fp32 accumulation, unrounded last layer) emulated in the restatement on the CPU
# differ from its fp32 run by 5.6e-3 to 6.1e-3 (rel L2, `vggish_det_weight` weights, `eval_waves` inputs: 5.7e-3 on the 2 s
# pair and 6.1e-3 on the 10 s clip below); the kernels round at slightly different points (padded first layer, accumulation
# order of K = 12288), hence twice the 5.6e-3-5.7e-3 figure.
VGGISH_REL_L2 = 1.2e-2
# The same emulation moves the distance by 3.3e-3 relative on a 16 x 10 s set with 16 kHz on both sides, and by 7.9e-4
# (119.150 -> 119.056) on exactly the files of the end-to-end test; the statistic leans on the centred part of the embeddings,
# where the emulation's error is 2.5e-2 against 6.0e-3 overall, hence about four times the larger emulated shift.
FAD_REL = 1.5e-2


@pytest.fixture(scope="module")
def vggish():
    sd = dict(VT.det_state_dict())
    sd["pproc.pca_eigen_vectors"] = torch.zeros(128, 128)        # a hub-built model carries the post-processor's tables
    sd["pproc.pca_means"] = torch.zeros(128, 1)
    m = E.VGGish(use_pca=False, use_activation=False).to(DEV)
    m.load_state_dict(sd, strict=True)
    return m.eval()


_REF = {}


def _reference(tag, B, L):
    if tag not in _REF:
        wav = cases.eval_waves("vggish." + tag, B, L)
        _REF[tag] = (wav, VT.forward(VT.det_state_dict(), wav.numpy()))
    return _REF[tag]


@pytest.mark.parametrize("H,W,C", [(96, 64, 64), (48, 32, 128), (24, 16, 256), (12, 8, 512), (13, 7, 8), (2, 2, 8)])
def test_maxpool2_equals_torch(H, W, C):
    """ctta_maxpool2 against F.max_pool2d on bf16 values, bit for bit; mixed signs and all-negative inputs (a maximum seeded
    with zero would return 0 there), odd sizes (the trailing row / column is dropped)."""
    B = 2
    for name, shift in (("mixed", 0.0), ("negative", -2.0)):
        x = bf16_round(det("vggish.pool." + name, (B, C, H, W), 4) + shift)
        y = torch.empty(B, H // 2, W // 2, C, dtype=torch.bfloat16, device=DEV)
        x_d = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)
        N.check(N.lib().ctta_maxpool2(N.ptr(x_d), N.ptr(y), B, H, W, C, N.stream_ptr()))
        sync()
        ref = F.max_pool2d(x, 2, 2)
        assert torch.equal(y.float().permute(0, 3, 1, 2).cpu(), ref), (H, W, C, name)
        if shift:
            assert float(ref.max()) < 0.0


def test_maxpool2_refuses_a_channel_count_off_the_vector_width():
    x = torch.zeros(2, 4, 4, 12, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        N.check(N.lib().ctta_maxpool2(N.ptr(x), N.ptr(x), 2, 4, 4, 12, N.stream_ptr()))


@pytest.mark.parametrize("L", [15600, 32000, 160000])
def test_frontend_matches_the_float64_definition(L):
    """ctta_wav_to_vggish_logmel against vggish_input.waveform_to_examples restated in float64 numpy: two clips, full scale,
    -60 dB and silence (exactly ln 0.01 up to the bound); the example count and the patch layout come with it."""
    B = 2
    L_ = N.lib()
    h = N.c_void_p()
    N.check(L_.ctta_vggish_frontend_create(B, L, h))
    try:
        wav = cases.eval_waves("vggish.fe", B, L)
        ne = VT.n_examples(L)
        for amp in (1.0, 1e-3, 0.0):
            x = (wav * amp).contiguous()
            ref = np.stack([VT.logmel_examples(w) for w in x.numpy()])                   # (B, ne, 96, 64)
            out = torch.full((B, ne * 96, 64), float("nan"), dtype=torch.float32, device=DEV)
            N.check(L_.ctta_wav_to_vggish_logmel(h, N.ptr(x.to(DEV)), B, L, N.ptr(out), N.stream_ptr()))
            sync()
            got = out.cpu().numpy().astype(np.float64).reshape(B, ne, 96, 64)
            err = float(np.abs(got - ref).max())
            print("vggish front end L=%d amp=%g: max abs log-mel error %.3e (range %.2f .. %.2f)"
                  % (L, amp, err, ref.min(), ref.max()))
            assert np.isfinite(got).all() and err < FRONTEND_MAX_ABS, (L, amp, err)
            if amp == 0.0:
                assert float(np.abs(got - np.log(0.01)).max()) < FRONTEND_MAX_ABS
        short = torch.zeros(B, 15599, device=DEV)
        with pytest.raises(RuntimeError):
            N.check(L_.ctta_wav_to_vggish_logmel(h, N.ptr(short), B, 15599, N.ptr(out), N.stream_ptr()))
    finally:
        L_.ctta_mel_frontend_destroy(h)


@pytest.mark.parametrize("tag,B,L,rows", [("short", 2, 32000, 4), ("clip", 1, 160000, 10)])
def test_embeddings_match_the_restatement(vggish, tag, B, L, rows):
    """`VGGish.forward` against the fp32 torch restatement with the deterministic weights: 2 s clips in a batch and one 10 s
    clip (10 examples, 38 frames unused)."""
    wav, ref = _reference(tag, B, L)
    with torch.no_grad():
        out = vggish(wav.to(DEV))
    sync()
    assert tuple(out.shape) == (rows, 128) and out.dtype == torch.float32 and tuple(ref.shape) == (rows, 128)
    err = rel_l2(out.cpu(), ref)
    print("vggish embeddings %s: rel_l2 %.3e" % (tag, err))
    assert err < VGGISH_REL_L2
    # the last Linear is not rounded to bf16
    assert float((out.cpu() - bf16_round(out.cpu())).abs().max()) > 0.0
    if B > 1:                                   # no coupling between the clips of a batch: clip-major rows, the same bits
        with torch.no_grad():
            one = vggish(wav[1:2].to(DEV))
        assert torch.equal(one, out[rows // B:])
    assert float(out.min()) < 0.0
    vggish.use_activation = True                # VGGish(use_activation=True) on the same weights: the final ReLU
    try:
        with torch.no_grad():
            assert torch.equal(vggish(wav.to(DEV)), out.clamp(min=0))
    finally:
        vggish.use_activation = False


def test_chunked_passes_give_the_rows_of_unchunked_ones(vggish):
    """54 clips of 10 s are 540 examples: the front end takes them as 51 + 3 clips and the network as 512 + 28 examples
    (`VGGish.MAX_EXAMPLES`).  Against the same clips in three passes of 18 (180 examples, no chunking).  Both sides round at
    the same points; launches of another size may sum in another order (tile, split-K), and a sum that moves by fp32 noise,
    2^-24 sqrt(K), flips the bf16 rounding (half-step 2^-9) of about 2^-24 sqrt(12288) / 2^-9 = 3e-3 of a layer's outputs by
    one step of 2^-8 relative: 2^-8 sqrt(3e-3) = 2e-4 per layer, 6e-4 over eight rounded layers in quadrature.  Bound 1e-3 overall;
    on the worst single clip 2^-8 = 3.9e-3, one bf16 step on every element; a row in the wrong place is an error of order 1."""
    B, L = 54, 160000
    assert vggish.n_examples(L) * B > vggish.MAX_EXAMPLES and B > vggish.MAX_EXAMPLES // vggish.n_examples(L)
    base = cases.eval_waves("vggish.chunk", 6, L)
    wav = torch.cat([base * (0.4 + 0.1 * r) for r in range(9)]).to(DEV)
    with torch.no_grad():
        out = vggish(wav)
        ref = torch.cat([vggish(wav[b0:b0 + 18]) for b0 in range(0, B, 18)])
    sync()
    assert tuple(out.shape) == (540, 128)
    per_clip = max(rel_l2(out[10 * b:10 * b + 10], ref[10 * b:10 * b + 10]) for b in range(B))
    print("vggish chunked vs unchunked: rel_l2 %.3e, worst clip %.3e" % (rel_l2(out, ref), per_clip))
    assert rel_l2(out, ref) < 1e-3 and per_clip < 2.0 ** -8


def test_vggish_state_dict_and_rejections(vggish):
    sd = dict(VT.det_state_dict())
    del sd["embeddings.4.bias"]
    with pytest.raises(RuntimeError):
        E.VGGish().load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError):
        E.VGGish(use_pca=True)
    vggish.train()
    try:
        with pytest.raises(RuntimeError):
            vggish(torch.zeros(1, 32000, device=DEV))
    finally:
        vggish.eval()
    with pytest.raises(RuntimeError):
        vggish(torch.zeros(1, 32000))                       # a host tensor: there is no CPU path
    with pytest.raises(ValueError):
        vggish(torch.zeros(1, 15599, device=DEV))           # no example


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def test_evaluation_helper_reports_the_frechet_audio_distance(golden, vggish, tmp_path):
    """EvaluationHelper.main with a `vggish_model`: 16 generated clips of 10 s at 16 kHz against 16 ground-truth clips at 48 kHz
    (decimated by striding), 160 examples per side for 128 dimensions; the distance against `calculate_fad` on the
    restatement's fp32 embeddings of the `load_audio_task` waveforms; every other key as without the model."""
    from scipy.io import wavfile
    g = golden("eval_suite")
    cnn14 = E.Cnn14(features_list=["2048", "logits"]).to(DEV)
    cnn14.load_state_dict(cases.cnn14_weights(g["cnn14_keys"], g["cnn14_shapes"]), strict=True)
    gen_dir, gt_dir = tmp_path / "gen", tmp_path / "gt"
    gen_dir.mkdir()
    gt_dir.mkdir()
    n = 16
    gen = cases.eval_waves("vggish.e2e.gen", n, 160000).numpy()
    gt = cases.eval_waves("vggish.e2e.gt", n, 480000, sr=48000).numpy()
    for i in range(n):
        wavfile.write(str(gen_dir / ("clip_%02d.wav" % i)), 16000, (gen[i] * 32767).astype(np.int16))
        wavfile.write(str(gt_dir / ("clip_%02d.wav" % i)), 48000, (gt[i] * 32767).astype(np.int16))
    res = E.EvaluationHelper(16000, DEV, mel_model=cnn14, vggish_model=vggish).main(None, str(gen_dir), str(gt_dir))
    assert list(res) == E.EvaluationHelper.KEYS
    fad = res["frechet_audio_distance"]
    assert np.isfinite(fad)
    names = ["clip_%02d.wav" % i for i in range(n)]
    sd = VT.det_state_dict()
    e_gen = VT.forward(sd, np.stack([E.load_audio_task(str(gen_dir / f)) for f in names]))
    e_gt = VT.forward(sd, np.stack([E.load_audio_task(str(gt_dir / f)) for f in names]))
    assert e_gen.shape[0] >= 129 and e_gt.shape[0] >= 129          # more rows than dimensions: non-singular covariances
    ref = E.calculate_fad(e_gen, e_gt)["frechet_audio_distance"]
    print("frechet_audio_distance: HIP %.4f, fp32 restatement %.6f, relative %.3e" % (fad, ref, abs(fad - ref) / abs(ref)))
    assert abs(fad - ref) <= FAD_REL * abs(ref)
    plain = E.EvaluationHelper(16000, DEV, mel_model=cnn14).main(None, str(gen_dir), str(gt_dir))
    assert np.isnan(plain["frechet_audio_distance"])
    for k in E.EvaluationHelper.KEYS:
        if k != "frechet_audio_distance":
            assert _same(res[k], plain[k]), (k, res[k], plain[k])
    os.remove(str(gen_dir / "clip_00.wav"))
    with pytest.raises(ValueError):
        E.EvaluationHelper(16000, DEV, mel_model=cnn14, vggish_model=vggish).main(None, str(gen_dir), str(gt_dir))
