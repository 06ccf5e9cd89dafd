"""The captured serving paths -- few-step sampling, post-CFG and tokens-in as one hipGraph, as the software pipeline, and
as the graphed student loop of AudioLCM.inference -- against this repository's own eager path, bit for bit (the eager path
is what tests/test_models_gpu.py and tests/test_solvers_gpu.py pin to the reference)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402
from consistencytta_amd import scheduler, spec  # noqa: E402

DEV = "cuda:0"
B, L, LATENT = 2, 7, (8, 32, 16)
W_IN = 4.0


class _WhitespaceTokenizer:
    """Whitespace tokenizer with T5's calling convention (the sentencepiece model is not available offline): ids in
    [2, 502), EOS = 1, pad = 0."""
    model_max_length = 512

    def __call__(self, prompt, max_length=None, padding=True, truncation=True, return_tensors="pt"):
        max_length = max_length or self.model_max_length
        rows = [[(sum(map(ord, w)) % 500) + 2 for w in p.split()][:max_length - 1] + [1] for p in prompt]
        width = max_length if padding == "max_length" else max(len(r) for r in rows)
        ids = torch.zeros(len(rows), width, dtype=torch.long)
        mask = torch.zeros(len(rows), width, dtype=torch.long)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = torch.tensor(r)
            mask[i, :len(r)] = 1
        return type("Batch", (), {"input_ids": ids, "attention_mask": mask})()


def _pipe(tokens=False):
    from consistencytta_amd import modules, text_encoder
    from consistencytta_amd.models import ConsistencyTTA
    cfg = dict(cases.TINY_UNET)
    kw = {}
    if tokens:
        cfg["cross_attention_dim"] = cases.TINY_T5["d_model"]
        te = text_encoder.T5EncoderModel(cases.TINY_T5)
        te.load_state_dict(cases.t5_weights(cases.TINY_T5))
        kw = dict(text_encoder=te, tokenizer=_WhitespaceTokenizer())
    vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    pipe = ConsistencyTTA(unet_config=cfg, vae=vae, **kw)
    pipe.to(DEV)
    pipe.unet.init_deterministic(1)
    vae.init_deterministic(2)
    pipe.eval().requires_grad_(False)
    return pipe, cfg


def _noise(steps, seed, batch=B):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((steps, batch) + LATENT, generator=g).to(DEV)


def _states(cfg, tag, Lx=L):
    _, _, _, enc, mask = cases.unet_inputs(cfg, B, LATENT[1], LATENT[2], Lx, tag)
    return enc.to(DEV), mask.to(DEV)


def _uncond(cfg, rows, tag, Lx=L):
    u = cases.t(spec.det_uniform(tag + ".unc", (rows, Lx, cfg["cross_attention_dim"]), 12)) * 0.5
    m = torch.zeros(rows, Lx, dtype=torch.bool)
    m[:, :2] = True
    return u.to(DEV), m.to(DEV)


def _eager(pipe, enc, mask, noise, post, steps, unc=None, unc_mask=None):
    """(latent, mel, int16) of the eager path on explicit draws: noise[0] the initial one, noise[1:] the step noise."""
    kw = {}
    if post > 1:
        kw = dict(uncond_states=unc.expand(B, -1, -1), uncond_mask=unc_mask.expand(B, -1))
    lat = pipe.generate_latent(enc, mask, noise[0], W_IN, post, steps, step_noise=noise[1:], **kw)
    mel = pipe.vae.decode_first_stage(lat.float())
    pcm = pipe.forward_from_embeds(enc, mask, noise[0], W_IN, post, steps, step_noise=noise[1:], **kw)
    assert np.array_equal(pcm, pipe.vae.decode_to_waveform(mel))
    return lat.clone(), mel.clone(), pcm


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------- 1: the kernel
def _renoise(cond, unc, w, nz, sig, copies, n, out):
    return N.lib().ctta_consistency_renoise(N.ptr(cond), N.ptr(unc), N.ptr(w) if w is not None else N.c_void_p(0), N.ptr(nz),
                                            N.ptr(sig), N.ptr(out), copies, cond.shape[0], n, N.stream_ptr())


@pytest.mark.parametrize("n", [4, 4 * 257, 4096])
def test_renoise_kernel_equals_the_unfused_sequence_bit_for_bit(n):
    """(1 - w) * u + w * c in torch, ctta_heun_add_noise, ctta_heun_scale_model_input, torch.cat -- the launches the eager
    sampler makes between two queries -- against the one-pass kernel: copies 1 and 2, with and without the uncond half,
    per-row w in {1, 2, 0.5} and per-row sigmas (sigma_max, 0, an inner one).  The output buffer starts as NaN and is
    followed by 256 sentinel floats: every element is written, nothing behind the tensor is."""
    L_ = N.lib()
    Bk = 3
    g = torch.Generator().manual_seed(n)
    c, u, nz = (torch.randn(Bk, n, generator=g).to(DEV) for _ in range(3))
    sig = torch.tensor([14.6146, 0.0, 0.7], dtype=torch.float32, device=DEV)
    w = torch.tensor([1.0, 2.0, 0.5], dtype=torch.float32, device=DEV)
    for use_unc in (False, True):
        x0 = ((1 - w[:, None]) * u + w[:, None] * c) if use_unc else c
        z, ref1 = torch.empty_like(c), torch.empty_like(c)
        N.check(L_.ctta_heun_add_noise(N.ptr(x0), N.ptr(nz), N.ptr(sig), N.ptr(z), Bk, n, N.stream_ptr()))
        N.check(L_.ctta_heun_scale_model_input(N.ptr(z), N.ptr(sig), N.ptr(ref1), Bk, n, N.stream_ptr()))
        assert bool(torch.isfinite(ref1).all())
        for copies in (1, 2):
            ref = torch.cat([ref1] * copies)
            buf = torch.full((copies * Bk * n + 256,), float("nan"), device=DEV)
            buf[copies * Bk * n:] = 12345.0
            N.check(_renoise(c, u if use_unc else None, w if use_unc else None, nz, sig, copies, n, buf))
            got = buf[:copies * Bk * n].view(copies * Bk, n)
            assert not bool(torch.isnan(got).any()), (use_unc, copies)
            assert torch.equal(_bits(got), _bits(ref)), (use_unc, copies)
            assert bool((buf[copies * Bk * n:] == 12345.0).all()), (use_unc, copies)


def test_renoise_kernel_refuses_a_row_length_that_is_no_multiple_of_four():
    Bk, n = 3, 6
    c, nz = torch.ones(Bk, n, device=DEV), torch.ones(Bk, n, device=DEV)
    sig = torch.ones(Bk, device=DEV)
    buf = torch.full((2 * Bk * n + 256,), float("nan"), device=DEV)
    assert _renoise(c, None, None, nz, sig, 2, n, buf) != 0
    with pytest.raises(N.CttaError, match="multiple of 4"):
        N.check(_renoise(c, None, None, nz, sig, 1, n, buf))
    with pytest.raises(N.CttaError):
        N.check(_renoise(c, None, None, nz, sig, 3, 8, buf))          # copies outside {1, 2}
    with pytest.raises(N.CttaError):
        N.check(_renoise(c, c, None, nz, sig, 1, 8, buf))             # uncond without w
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())                               # nothing was launched


# ------------------------------------------------------------------------------------- 2: step_noise on the eager path
def test_explicit_step_noise_reproduces_the_internal_draws():
    pipe, cfg = _pipe()
    enc, mask = _states(cfg, "serve2")
    noise = _noise(1, 20)[0]
    torch.manual_seed(11)
    a = pipe.generate_latent(enc, mask, noise, W_IN, 1.0, 3)
    torch.manual_seed(11)
    draws = torch.stack([torch.randn_like(noise), torch.randn_like(noise)])     # today's calls, in today's order
    b = pipe.generate_latent(enc, mask, noise, W_IN, 1.0, 3, step_noise=draws)
    assert torch.equal(_bits(a), _bits(b))
    c = pipe.generate_latent(enc, mask, noise, W_IN, 1.0, 3, step_noise=draws.flip(0))
    assert not torch.equal(a, c)                                                # the draws are really used


# -------------------------------------------------------------------------------------------------- 3: capture_graph
@pytest.mark.parametrize("steps,post,unc_rows", [(2, 1.0, 0), (3, 2.0, 1), (1, 2.0, B), (2, 1.3, B)])
def test_captured_graph_equals_eager_few_step_and_post_cfg(steps, post, unc_rows):
    """post = 1.3: 1 - w is not exact in fp32, where the kernels' fp32 subtraction and torch's rounded double differ in the last
    bit -- the capture keeps torch's own combine there (models._post_cfg_fusable) and stays bit-identical."""
    from consistencytta_amd.models import _post_cfg_fusable
    assert _post_cfg_fusable(2.0) and _post_cfg_fusable(2.5) and not _post_cfg_fusable(1.3)
    pipe, cfg = _pipe()
    unc, unc_mask = _uncond(cfg, unc_rows, "serve3") if unc_rows else (None, None)
    inputs = [_states(cfg, "serve3_%d" % i) + (_noise(steps, 30 + i),) for i in range(2)]
    refs = [_eager(pipe, e, m, nz, post, steps, unc, unc_mask) for e, m, nz in inputs]
    assert not np.array_equal(refs[0][2], refs[1][2])
    gen = pipe.capture_graph(B, L, cfg_scale_input=W_IN, cross_attention_dim=cfg["cross_attention_dim"], latent=LATENT,
                             num_steps=steps, cfg_scale_post=post, uncond_states=unc, uncond_mask=unc_mask)
    for (e, m, nz), (lat, mel, pcm) in zip(inputs, refs):
        out = gen(e, m, nz)
        assert torch.equal(_bits(gen.outputs[0]), _bits(lat))
        assert torch.equal(_bits(gen.outputs[1]), _bits(mel))
        assert np.array_equal(out.cpu().numpy(), pcm)
    if steps > 1:
        with pytest.raises(ValueError):
            gen(inputs[0][0], inputs[0][1], inputs[0][2][0])          # a (B, C, H, W) noise where num_steps rows are due


# ----------------------------------------------------------------------------------------------- 4: capture_pipeline
def test_pipeline_two_step_post_cfg_returns_each_batch_two_calls_later():
    pipe, cfg = _pipe()
    steps, post = 2, 2.0
    unc, unc_mask = _uncond(cfg, B, "serve4")
    batches = [_states(cfg, "serve4_%d" % i) + (_noise(steps, 40 + i),) for i in range(5)]
    refs = [_eager(pipe, e, m, nz, post, steps, unc, unc_mask)[2] for e, m, nz in batches]
    assert not np.array_equal(refs[0], refs[1])
    gen = pipe.capture_pipeline(B, L, cfg_scale_input=W_IN, cross_attention_dim=cfg["cross_attention_dim"], latent=LATENT,
                                candidates=3, num_steps=steps, cfg_scale_post=post, uncond_states=unc, uncond_mask=unc_mask)
    assert gen.depth == 2 and set(gen.placement_ms) == {"u", "v"}
    outs = [gen(*b).cpu().numpy().copy() for b in batches + batches[-1:] * 2]      # two extra calls drain the pipeline
    for j, ref in enumerate(refs):
        assert np.array_equal(outs[j + 2], ref), j


# --------------------------------------------------------------------------------------------------- 5: tokens in
PROMPTS = [["a dog barks twice near the mill", ""], ["rain", "birds sing while a train passes by"],
           ["", "wind"], ["a siren then a crash of glass", "footsteps on gravel"]]
LT = 8      # the longest prompts: 7 words + EOS


def _token_refs(pipe, steps, post, seeds):
    toks, refs = [], []
    for p, s in zip(PROMPTS, seeds):
        tok = pipe.tokenizer(p, max_length=LT, padding="max_length")
        enc, mask = pipe.encode_text(p, max_length=LT, padding="max_length")
        nz = _noise(steps, s)
        kw = {}
        if post > 1:
            cf, mcf, _, _ = pipe.encode_text_classifier_free(PROMPTS[0], 1)      # its longest prompt fills the bucket
            assert cf.shape[1] == LT
            kw = dict(uncond_states=cf[:B], uncond_mask=mcf[:B])
        lat = pipe.generate_latent(enc, mask, nz[0], W_IN, post, steps, step_noise=nz[1:], **kw)
        pcm = pipe.forward_from_embeds(enc, mask, nz[0], W_IN, post, steps, step_noise=nz[1:], **kw)
        toks.append((tok.input_ids, tok.attention_mask, nz))
        refs.append((lat.clone(), pcm, kw))
    return toks, refs


def test_tokens_in_graph_equals_text_encoder_then_eager():
    pipe, cfg = _pipe(tokens=True)
    steps, post = 2, 2.0
    toks, refs = _token_refs(pipe, steps, post, (50, 51, 52, 53))
    assert int(toks[0][1][1].sum()) == 1 and int(toks[0][1][0].sum()) == LT     # a single-token row beside a full one
    gen = pipe.capture_graph(B, LT, cfg_scale_input=W_IN, cross_attention_dim=cfg["cross_attention_dim"], latent=LATENT,
                             num_steps=steps, cfg_scale_post=post, from_tokens=True)
    assert torch.equal(_bits(gen.uncond_states), _bits(refs[0][2]["uncond_states"]))
    assert torch.equal(gen.uncond_mask, refs[0][2]["uncond_mask"])
    for i, ((ids, am, nz), (lat, pcm, _)) in enumerate(zip(toks, refs)):
        if i % 2:                                        # tokens already on the device take the unchecked route
            ids, am = ids.to(DEV), am.to(DEV)
        out = gen(ids, am, nz)
        assert torch.equal(_bits(gen.outputs[0]), _bits(lat)), i
        assert np.array_equal(out.cpu().numpy(), pcm), i
    bad = toks[0][0].clone()
    bad[0, 0] = cases.TINY_T5["vocab_size"]
    with pytest.raises(IndexError):
        gen(bad, toks[0][1], toks[0][2])
    with pytest.raises(ValueError):
        gen(toks[0][0][:, :-1], toks[0][1][:, :-1], toks[0][2])


def test_tokens_in_pipeline_is_four_stages_and_returns_each_batch_three_calls_later():
    pipe, cfg = _pipe(tokens=True)
    toks, refs = _token_refs(pipe, 1, 1.0, (60, 61, 62, 63))
    assert not np.array_equal(refs[0][1], refs[1][1])
    gen = pipe.capture_pipeline(B, LT, cfg_scale_input=W_IN, cross_attention_dim=cfg["cross_attention_dim"], latent=LATENT,
                                candidates=3, from_tokens=True)
    assert gen.depth == 3 and set(gen.placement_ms) == {"u", "v", "t"} and len(gen.graphs) == 4
    outs = [gen(ids, am, nz[0]).cpu().numpy().copy() for ids, am, nz in toks + toks[-1:] * 3]      # three calls drain it
    for j, (_, pcm, _) in enumerate(refs):
        assert np.array_equal(outs[j + 3], pcm), j


# ------------------------------------------------------------------------------------ 6: AudioLCM's graphed student loop
def _lcm(use_edm):
    from consistencytta_amd.models import AudioLCM
    cfg = cases.TINY_UNET
    m = AudioLCM(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                 unet_model_config_path="tiny_light.json", unet_config=cfg, snr_gamma=5.0, use_edm=use_edm,
                 teacher_guidance_scale=-1, num_diffusion_steps=18, vae=None, loss_type="mse")
    m.student_target_unet.load_state_dict(cases.unet_weights(cfg, True, 2))
    m.student_ema_unet.load_state_dict(cases.unet_weights(cfg, True, 3))
    m.to(DEV)
    m.eval()
    P = {k: v.to(DEV) for k, v in cases.prompt_states(cfg, B, 6, "serve6").items()}
    return m, P


@pytest.mark.parametrize("heun,steps,post,use_ema", [(True, 1, 1.0, True), (True, 1, 2.0, False), (True, 2, 1.0, False),
                                                      (True, 2, 2.0, True), (True, 3, 1.3, True), (False, 4, 1.0, True),
                                                      (False, 4, 2.0, False)])
def test_graphed_student_loop_equals_the_eager_loop(heun, steps, post, use_ema):
    m, P = _lcm(use_edm=heun)
    cls = scheduler.HeunDiscreteScheduler if heun else scheduler.DDIMScheduler
    sched = cls.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    nz = _noise(steps, 70 + steps)
    kw = dict(guidance_scale_input=W_IN, guidance_scale_post=post, num_steps=steps, use_ema=use_ema, noise=nz[0])
    eager = m.inference(P, sched, step_noise=nz[1:], **kw)
    graphed = m.inference(P, sched, step_noise=nz[1:], graph_student=True, **kw)
    assert torch.equal(_bits(eager), _bits(graphed))
    again = m.inference(P, sched, step_noise=nz[1:], graph_student=True, **kw)      # a fresh capture on a warm handle
    assert torch.equal(_bits(eager), _bits(again))
    if steps > 1:
        torch.manual_seed(3)
        e2 = m.inference(P, sched, **kw)
        torch.manual_seed(3)
        g2 = m.inference(P, sched, graph_student=True, **kw)                        # the internal draws, in their order
        assert torch.equal(_bits(e2), _bits(g2)) and not torch.equal(e2, eager)
        with pytest.raises(ValueError, match="step_noise"):
            m.inference(P, sched, step_noise=nz, graph_student=True, **kw)


# ------------------------------------------------------------------------------------------- 7: the old call signatures
def test_old_positional_arguments_still_give_the_single_step_callables():
    pipe, cfg = _pipe()
    batches = [_states(cfg, "serve7_%d" % i) + (_noise(1, 80 + i)[0],) for i in range(3)]
    refs = [pipe.forward_from_embeds(e, m, nz, W_IN, 1.0, 1) for e, m, nz in batches]
    gen = pipe.capture_graph(B, L, W_IN, cfg["cross_attention_dim"], LATENT)
    for b, ref in zip(batches, refs):
        assert b[2].shape == (B,) + LATENT
        assert np.array_equal(gen(*b).cpu().numpy(), ref)
    gen3 = pipe.capture_pipeline(B, L, W_IN, cfg["cross_attention_dim"], LATENT, 3)
    assert gen3.depth == 2
    outs = [gen3(*b).cpu().numpy().copy() for b in batches + batches[-1:] * 2]
    for j, ref in enumerate(refs):
        assert np.array_equal(outs[j + 2], ref), j
