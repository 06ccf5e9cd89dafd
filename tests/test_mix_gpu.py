"""The mix augmentation of the training batch on the GPU (csrc/mix_augment.hip via consistencytta_amd/data.py) against
the reference's own tools.mix / tools.torch_tools.augment (tests/golden/mix_augment.npz, make_golden_mix.py)."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
import make_golden_mix as mgm  # noqa: E402
from consistencytta_amd import data, modules  # noqa: E402
from gpu_util import DEV  # noqa: E402

GAIN_DB_TOL = 1e-3
T_TOL = 1e-5
MIX_TOL = 1e-5


def _wave_a():
    return mgm.test_wave(6, mgm.L_A, "mixA", mgm.KINDS_A)


def _wave_b():
    return mgm.test_wave(2, mgm.L_B, "mixB", mgm.KINDS_B)


def _strs(a):
    return [str(s) for s in a]


@pytest.mark.parametrize("mode,fs,key", [("A_weighting", 16000, "gain_a16k"), ("A_weighting", 44100, "gain_a44k"),
                                         ("RMSE", 16000, "gain_rmse16k"), ("RMSE", 44100, "gain_rmse44k")])
def test_frame_gains_match_reference(golden, mode, fs, key):
    g = golden("mix_augment")
    ref = g[key]
    got = data.compute_gain(_wave_a().to(DEV), fs, mode=mode)
    assert torch.is_tensor(got) and got.is_cuda and tuple(got.shape) == ref.shape
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    print("%s @ %d Hz: max |gain - ref| = %.3e dB (per clip %s)" % (mode, fs, err.max(), err.max(1)))
    assert err.max() <= GAIN_DB_TOL
    assert np.abs(got[3].cpu().numpy() + 80.0).max() <= 1e-5                # the silent clip sits at min_db
    one = data.compute_gain(_wave_a()[1].numpy(), fs, mode=mode)          # numpy in -> numpy float64 out, 1-D
    assert isinstance(one, np.ndarray) and one.dtype == np.float64 and one.shape == ref[1].shape
    assert np.abs(one - ref[1]).max() <= GAIN_DB_TOL                        # the low-frequency clip


def test_frame_gains_of_a_full_clip(golden):
    g = golden("mix_augment")
    got = data.compute_gain(_wave_b(), 16000)                              # CPU tensor in -> CPU tensor out
    assert torch.is_tensor(got) and not got.is_cuda
    assert float(np.abs(got.numpy().astype(np.float64) - g["gain_b_a16k"]).max()) <= GAIN_DB_TOL


@pytest.mark.parametrize("k", [0, 1])
def test_augment_matches_reference(golden, k):
    g = golden("mix_augment")
    texts = _strs(g["texts_a"])
    wav = _wave_a().to(DEV)
    random.seed(int(g["seeds_a"][k]))
    mixed, caps = data.augment(wav, texts, num_items=3)
    assert caps == _strs(g["a%d_captions" % k])
    assert mixed.dtype == torch.float32 and mixed.is_cuda and tuple(mixed.shape) == (3, mgm.L_A)
    got = mixed.cpu().numpy()
    if k == 1:
        got = got[:, ::4]
    err = float(np.abs(got - g["a%d_mix" % k]).max())
    print("case A seed %d: mixtures max abs err %.3e" % (int(g["seeds_a"][k]), err))
    assert err <= MIX_TOL
    # t and the clip gains of each pair
    pairs = torch.from_numpy(g["a%d_pairs" % k]).to(DEV)
    t = torch.empty(3, device=DEV)
    gg = torch.empty(3, 2, device=DEV)
    dst = torch.empty(3, mgm.L_A, device=DEV)
    data.mixer(DEV).mix(wav, pairs, dst, groups=1, t_out=t, g_out=gg)
    assert float(np.abs(t.cpu().numpy() - g["a%d_t" % k]).max()) <= T_TOL
    assert float(np.abs(gg.cpu().numpy() - g["a%d_g" % k]).max()) <= GAIN_DB_TOL
    assert torch.equal(dst, mixed)


def test_collate_full_clips_matches_reference(golden):
    g = golden("mix_augment")
    texts = _strs(g["texts_b"])
    wav = _wave_b().to(DEV)
    random.seed(7)
    caps, out = data.collate(texts, wav)
    assert caps == texts + _strs(g["b_captions"])
    assert tuple(out.shape) == (3, mgm.L_B)
    assert torch.equal(out[:2], wav)                                       # source rows unchanged, bit for bit
    m = out[2].cpu().numpy()
    err = max(float(np.abs(m[:32768] - g["b_mix_head"]).max()), float(np.abs(m[::8] - g["b_mix_sub"]).max()))
    print("case B (10.24 s): mixture max abs err %.3e" % err)
    assert err <= MIX_TOL
    t = torch.empty(1, device=DEV)
    data.mixer(DEV).mix(wav, torch.tensor([[0, 1]], dtype=torch.int32, device=DEV), torch.empty(1, mgm.L_B, device=DEV),
                        t_out=t)
    assert abs(float(t[0]) - float(g["b_t"][0])) <= T_TOL
    # the unnormalised pair mix (tools/mix.py's mix) normalises to the same row
    raw, cap = data.mix_wavs_and_captions(wav[0], wav[1], texts[0], texts[1])
    assert cap == str(g["b_captions"][0]) and tuple(raw.shape) == (1, mgm.L_B)
    assert float((raw[0] / raw.abs().max() / 2 - out[2]).abs().max()) <= 1e-6


def test_two_groups_in_one_call_equal_two_collates():
    wa = _wave_a()
    w = torch.cat([wa, 0.7 * wa.roll(1, 0).flip(1)]).to(DEV)
    caps = ["clip %d" % i for i in range(12)]
    random.seed(11)
    c_fused, fused = data.collate(caps, w, groups=2)
    random.seed(11)
    c0, o0 = data.collate(caps[:6], w[:6])
    c1, o1 = data.collate(caps[6:], w[6:])
    assert tuple(fused.shape) == (18, mgm.L_A)
    assert torch.equal(fused[:12], w)
    assert torch.equal(fused[12:15], o0[6:]) and torch.equal(fused[15:], o1[6:])
    assert c_fused == caps + c0[6:] + c1[6:]


def test_all_silent_batch_is_nan_like_the_reference():
    caps, out = data.collate(["Silence", "more silence"], torch.zeros(2, 8192, device=DEV))
    assert caps[2] == "Silence and more silence"
    assert torch.equal(out[:2], torch.zeros(2, 8192, device=DEV))
    assert bool(torch.isnan(out[2]).all())


def test_collate_captured_in_a_graph_equals_eager():
    B, L = 6, mgm.L_A
    wa = _wave_a().to(DEV)
    wb = (0.5 * wa.flip(0).roll(777, 1)).contiguous()
    caps = ["c%d" % i for i in range(B)]
    static_wav = wa.clone()
    static_pairs = torch.tensor([[0, 2], [1, 4], [3, 5]], dtype=torch.int32, device=DEV)
    static_out = torch.empty(B + 3, L, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        data.collate(caps, static_wav, out=static_out, pairs=static_pairs)      # warm-up: the handle is sized here
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        data.collate(caps, static_wav, out=static_out, pairs=static_pairs)
    new_pairs = [(5, 1), (2, 3), (0, 4)]
    static_wav.copy_(wb)
    static_pairs.copy_(torch.tensor(new_pairs, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    eager_caps, eager = data.collate(caps, wb, pairs=new_pairs)
    assert eager_caps[B:] == ["c5 and c1", "c2 and c3", "c0 and c4"]
    assert torch.equal(static_out, eager)
    assert not torch.equal(eager[B:], data.collate(caps, wa, pairs=new_pairs)[1][B:])   # the replay did use the new input


def _lcm():
    from consistencytta_amd.models import AudioLCM
    cfg = cases.TINY_UNET
    m = AudioLCM(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                 unet_model_config_path="tiny_light.json", unet_config=cfg, snr_gamma=5.0, use_edm=True,
                 teacher_guidance_scale=-1, num_diffusion_steps=18, vae=None, loss_type="mse",
                 target_ema_decay=0.95, ema_decay=0.999)
    m.teacher_unet.load_state_dict(cases.unet_weights(cfg, False, 0))
    m.student_unet.load_state_dict(cases.unet_weights(cfg, True, 1))
    m.student_target_unet.load_state_dict(cases.unet_weights(cfg, True, 2))
    m.student_ema_unet.load_state_dict(cases.unet_weights(cfg, True, 3))
    m.to(DEV)
    P = {k: v.to(DEV) for k, v in cases.prompt_states(cfg, 3, 6, "distill").items()}
    return m, P


def test_training_step_on_a_mixed_batch_matches_reference_mixture(golden):
    """collate -> wav_to_fbank -> VAE encode -> one AudioLCM distillation step (the tiny-width setup of
    test_train_gpu.test_real_training_step_from_waveforms), against the same step fed the reference's mixture."""
    from consistencytta_amd import audio
    g = golden("mix_augment")
    d = golden("distill_tiny")
    dd = cases.TINY_VAE_DD
    vae = modules.AutoencoderKL(ddconfig=dd, embed_dim=8, scale_factor=0.9227914214134216, hifigan_config=cases.TINY_HIFIGAN)
    sd = dict(cases.vae_weights(dd))
    sd.update(cases.vae_encoder_weights(dd))
    sd.update(cases.hifigan_weights(cases.TINY_HIFIGAN))
    vae.load_state_dict(sd)
    vae.to(DEV).eval().requires_grad_(False)
    stft = audio.TacotronSTFT(1024, 160, 1024, 32, 16000, 0, 8000).to(DEV)

    wav = _wave_b().to(DEV)
    random.seed(7)
    _, batch = data.collate(_strs(g["texts_b"]), wav)
    ours = batch[:, :32768].contiguous()
    ref = torch.cat([wav[:, :32768], torch.from_numpy(g["b_mix_head"])[None].to(DEV)]).contiguous()
    losses = []
    for w in (ours, ref):
        torch.manual_seed(0)                         # the posterior sample of get_first_stage_encoding draws randn
        with torch.no_grad():
            mel, _ = audio.wav_to_fbank(w, 128, stft)
            z0 = vae.get_first_stage_encoding(vae.encode_first_stage(mel.unsqueeze(1)))
        assert tuple(z0.shape) == (3, 8, 32, 8) and bool(torch.isfinite(z0).all())
        m, P = _lcm()
        m.train()
        opt = m.prepare_training(lr=1e-5, weight_decay=1e-4, broadcast=False)
        draws = dict(time_inds=torch.from_numpy(d["time_inds"]) * 2, gaussian_noise=torch.from_numpy(d["noise"]).to(DEV),
                     guidance_scale=torch.from_numpy(d["guidance"]))
        losses.append(m.train_step(z0, P, opt, None, **draws))
    print("loss on the HIP-mixed batch %.8f, on the reference-mixed batch %.8f" % tuple(losses))
    assert losses[0] == losses[0] and losses[0] > 0
    assert abs(losses[0] - losses[1]) <= 1e-4 * abs(losses[1])
