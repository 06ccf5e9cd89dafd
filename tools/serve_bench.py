#!/usr/bin/env python3
"""Serving forms of ConsistencyTTA side by side, in one process on one GPU, at BASELINE.json configs[1]'s size and built
the way bench.py builds its pipeline (light U-Net, full VAE + HiFi-GAN, batch 32, L = 32, FLAN-T5-large's shape, random
init):

  (a) states_pipeline        the states-in 3-stage pipeline bench.py times -- the control
  (b) eager_t5_then_pipeline T5EncoderModel.forward on the batch's tokens (cond only), then (a): the best prompt-in form
                             without a captured text encoder
  (c) tokens_pipeline        capture_pipeline(from_tokens=True): FLAN-T5 as a fourth graph on a fourth stream
  (d) num_steps = 2, and num_steps = 2 with cfg_scale_post = 2: eager launches, one hipGraph, the pipeline

Every form gets host tokens / device states of the same batch and is checked against its eager counterpart (bit for bit)
before anything is timed.  Timing: all forms are warmed up, then measured in ROUNDS that alternate them (one window of
`--steps` calls per form per round, host clock around work that ends in a device synchronise), so a drift of the box hits
every form alike; the JSON keeps every window, the median and the ratios of medians:

  c_over_b   whether the tokens-in pipeline pays            (< 1: faster than eager T5 + pipeline)
  c_over_a   how much of the encoder is left visible        (1.0: hidden entirely)
  graph_over_eager / pipeline_over_eager for the few-step forms

  python tools/serve_bench.py --out profiles/serve_bench.json

`--edit` runs another leg alone (no text encoder): the captured edit path beside the captured plain few-step path at
`--edit-steps` queries, and the one-pass step kernel beside the launches it replaces (see `edit_leg`):

  python tools/serve_bench.py --edit --out profiles/edit_serving.json

`--long [--duration 30.72]` runs the long-clip leg alone: the captured long path (8 clips x 4 windows by default) beside the
captured plain few-step path at the same number of U-Net rows (batch 32), and the one-pass window step beside the launches
it replaces (see `long_leg`):

  python tools/serve_bench.py --long --out profiles/long_serving.json

`--long-edit [--duration 30.72 --source-seconds 10.24]` runs the long-edit leg alone: the captured long edit (a source kept
at the start of every clip, the rest generated) beside the captured plain long path at the same clips and windows, and the
one-pass edit step beside the launches it replaces (see `long_edit_leg`):

  python tools/serve_bench.py --long-edit --out profiles/long_edit_serving.json

`--seeded` runs the seeded leg alone: the seeded captures (seeds in, the Philox fill at the head of the graph) beside the
plain captures fed a device `torch.randn` per call, at the plain mode's shape and at the long leg's, and the fill launch
beside the draws and uploads it replaces (see `seeded_leg`):

  python tools/serve_bench.py --seeded --out profiles/seeded_serving.txt

`--adapters` runs the adapter leg alone: a batch whose rows ask for four different LoRA adapters (one captured graph, the
adapter looked up per row) beside the plain path, the single-adapter path and four quarter-batch replays with an
adapter reload in front of each (see `adapters_leg`):

  python tools/serve_bench.py --adapters --out profiles/lora_mixed.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def edit_leg(args):
    """`--edit`: the captured edit path (capture_edit_graph: inpainting with a (0.25, 0.75) time mask) beside the captured
    plain few-step path (capture_graph) at the same num_steps, states in, in alternating windows; and the one-pass step
    kernel (ctta_consistency_edit_renoise) beside the launches it replaces (torch combine, torch blend,
    ctta_heun_add_noise, ctta_heun_scale_model_input, torch.cat) on one latent-sized batch.  The source latent is
    synthetic: the waveform -> latent half runs eagerly before a replay and is not part of either form."""
    import torch
    from consistencytta_amd import _native as N
    from consistencytta_amd import modules, spec
    from consistencytta_amd.models import ConsistencyTTA
    dev = "cuda:0"
    B, L, steps = args.batch, args.text_len, args.edit_steps
    if args.tiny:
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        import cases
        ucfg, latent = dict(cases.TINY_UNET), (8, 32, 16)
        vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    else:
        ucfg, latent = spec.LIGHT_UNET_CONFIG, (8, 256, 16)
        vae = modules.AutoencoderKL(ddconfig=spec.VAE_DDCONFIG, embed_dim=8, scale_factor=0.9227914214134216)
    D = ucfg["cross_attention_dim"]
    pipe = ConsistencyTTA(unet_config=ucfg, vae=vae)
    pipe.to(dev)
    pipe.unet.init_random_(seed=0)
    vae.init_random_(seed=1)
    pipe.eval().requires_grad_(False)
    W_IN = 4.0
    g = torch.Generator(device="cpu").manual_seed(3)
    keep = pipe.latent_keep_mask(B, latent[1:], time_mask_ratio_start_and_end=(0.25, 0.75)).to(dev)
    batches = []
    for _ in range(2):
        lens = torch.randint(min(6, L), L + 1, (B,), generator=g)
        batches.append({"enc": (torch.randn(B, L, D, generator=g) * 0.25).to(dev),
                        "mask": (torch.arange(L)[None, :] < lens[:, None]).to(dev),
                        "noise": torch.randn((steps, B) + latent, generator=g).to(dev),
                        "src": (torch.randn((B,) + latent, generator=g) * 0.8).to(dev)})
    scratch = torch.empty(4, dtype=torch.float32, device=dev)

    def to_pcm(lat):
        wav = vae.vocode(vae.decode_first_stage(lat))
        pcm = torch.empty(wav.shape, dtype=torch.int16, device=dev)
        N.check(N.lib().ctta_wav_finalize(N.ptr(wav), wav.numel(), N.ptr(scratch), None, N.ptr(pcm), N.stream_ptr()))
        return pcm

    def eager_plain(b):
        return to_pcm(pipe.generate_latent(b["enc"], b["mask"], b["noise"][0], W_IN, 1.0, steps, step_noise=b["noise"][1:]))

    def eager_edit(b):
        return to_pcm(pipe.edit_latent(b["enc"], b["mask"], b["noise"][0], b["src"], keep, 1.0, W_IN, 1.0, steps,
                                       step_noise=b["noise"][1:]))

    ref_plain, ref_edit = eager_plain(batches[0]).clone(), eager_edit(batches[0]).clone()
    torch.cuda.synchronize()
    kw0 = dict(cfg_scale_input=W_IN, cross_attention_dim=D, latent=latent, num_steps=steps)
    gen_plain = pipe.capture_graph(B, L, **kw0)
    gen_edit = pipe.capture_edit_graph(B, L, **kw0)
    b0 = batches[0]
    parity = {"plain_graph": bool(torch.equal(gen_plain(b0["enc"], b0["mask"], b0["noise"]), ref_plain)),
              "edit_graph": bool(torch.equal(gen_edit(b0["enc"], b0["mask"], b0["noise"], b0["src"], keep), ref_edit))}
    if not all(parity.values()):
        raise SystemExit("a captured form differs from its eager counterpart: %s" % parity)

    turn = [0]

    def nxt():
        turn[0] ^= 1
        return batches[turn[0]]

    def plain_call():
        b = nxt()
        return gen_plain(b["enc"], b["mask"], b["noise"])

    def edit_call():
        b = nxt()
        return gen_edit(b["enc"], b["mask"], b["noise"], b["src"], keep)
    forms = {"plain_graph": plain_call, "edit_graph": edit_call, "plain_eager": lambda: eager_plain(nxt()),
             "edit_eager": lambda: eager_edit(nxt())}
    for fn in forms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    windows = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            windows[k].append((time.perf_counter() - t0) / args.steps * 1e3)
    med = {k: statistics.median(v) for k, v in windows.items()}

    # ---- the step between two queries alone: one launch against the chain it replaces, device time by events
    n, hw = latent[0] * latent[1] * latent[2], latent[1] * latent[2]
    c, u, nz, src = (torch.randn(B, n, generator=g).to(dev) for _ in range(4))
    sig = torch.full((B,), 0.7, device=dev)
    w = torch.full((B,), 2.0, device=dev)
    keep2 = keep.reshape(B, hw).contiguous()
    keep_rows = keep2[:, None, :].expand(B, latent[0], hw).reshape(B, n).contiguous()
    L_ = N.lib()

    def chain(cfg):
        x0 = ((1 - 2.0) * u + 2.0 * c) if cfg else c
        x0 = keep_rows * src + (1 - keep_rows) * x0
        z, out = torch.empty_like(x0), torch.empty_like(x0)
        N.check(L_.ctta_heun_add_noise(N.ptr(x0), N.ptr(nz), N.ptr(sig), N.ptr(z), B, n, N.stream_ptr()))
        N.check(L_.ctta_heun_scale_model_input(N.ptr(z), N.ptr(sig), N.ptr(out), B, n, N.stream_ptr()))
        return torch.cat([out] * 2) if cfg else out

    def fused(cfg):
        out = torch.empty((2 * B if cfg else B, n), device=dev)
        N.check(L_.ctta_consistency_edit_renoise(N.ptr(c), N.ptr(u) if cfg else N.c_void_p(0),
                                                 N.ptr(w) if cfg else N.c_void_p(0), N.ptr(src), N.ptr(keep2), N.ptr(nz),
                                                 N.ptr(sig), N.ptr(out), 2 if cfg else 1, B, n, hw, N.stream_ptr()))
        return out
    step_parity = {("cfg" if cfg else "cond"): bool(torch.equal(chain(cfg).view(torch.int32), fused(cfg).view(torch.int32)))
                   for cfg in (False, True)}
    step_forms = {"chain_cond": lambda: chain(False), "fused_cond": lambda: fused(False),
                  "chain_cfg": lambda: chain(True), "fused_cfg": lambda: fused(True)}
    step_us = {k: [] for k in step_forms}
    reps = 200
    for _ in range(args.rounds + 1):           # the first round warms up and is dropped
        for k, fn in step_forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            step_us[k].append(e0.elapsed_time(e1) / reps * 1e3)
    step_med = {k: statistics.median(v[1:]) for k, v in step_us.items()}
    result = {
        "tool": "tools/serve_bench.py --edit", "device": torch.cuda.get_device_name(0), "tiny": bool(args.tiny),
        "batch": B, "text_len": L, "latent": list(latent), "num_steps": steps, "time_mask_ratio_start_and_end": [0.25, 0.75],
        "steps_per_window": args.steps, "rounds": args.rounds, "warmup_calls": args.warmup,
        "unit": "ms per call of one batch; step kernels: us per step, stream time by events over %d back-to-back steps "
                "(launch cost included)" % reps,
        "timing": "host clock around a window of calls ending in a device synchronise; forms alternate within a round",
        "parity_bit_identical_to_eager": parity, "step_parity_bit_identical": step_parity,
        "ms_per_call_median": {k: round(v, 3) for k, v in med.items()},
        "ms_per_call_windows": {k: [round(x, 3) for x in v] for k, v in windows.items()},
        "ratios_of_medians": {"edit_graph_over_plain_graph": round(med["edit_graph"] / med["plain_graph"], 4),
                              "edit_eager_over_plain_eager": round(med["edit_eager"] / med["plain_eager"], 4),
                              "edit_graph_over_edit_eager": round(med["edit_graph"] / med["edit_eager"], 4)},
        "step_us_median": {k: round(v, 2) for k, v in step_med.items()},
        "step_us_windows": {k: [round(x, 2) for x in v[1:]] for k, v in step_us.items()},
        "step_fused_over_chain": {"cond": round(step_med["fused_cond"] / step_med["chain_cond"], 4),
                                  "cfg": round(step_med["fused_cfg"] / step_med["chain_cfg"], 4)},
    }
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


def long_leg(args):
    """`--long`: the captured long-clip path (capture_long_graph: `--long-clips` clips of `--duration` seconds, each queried
    as n overlapping windows) beside the captured plain few-step path (capture_graph) at the SAME number of U-Net rows
    (clips x windows clips of the model's own length), states in, at `--edit-steps` queries, in alternating windows; the
    eager forms of both; and the one-pass step kernel (ctta_window_fuse_renoise) beside the launches it replaces (torch
    combine, slices, torch weighted sum, ctta_heun_add_noise, ctta_heun_scale_model_input, the cut into windows,
    torch.cat) on one long batch.  The two paths decode different extents (clips x Ht rows against clips x windows x
    window rows); the JSON names both."""
    import torch
    from consistencytta_amd import _native as N
    from consistencytta_amd import modules, spec
    from consistencytta_amd.models import ConsistencyTTA, _long_latent_h
    dev = "cuda:0"
    Bl, L, steps = args.long_clips, args.text_len, args.edit_steps
    if args.tiny:
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        import cases
        ucfg, (C, wh, W), overlap = dict(cases.TINY_UNET), (8, 32, 16), 8
        duration = args.duration if args.duration is not None else 3.0
        make_vae = lambda: modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9,      # noqa: E731
                                                 hifigan_config=cases.TINY_HIFIGAN)
    else:
        ucfg, (C, wh, W), overlap = spec.LIGHT_UNET_CONFIG, (8, 256, 16), 64
        duration = args.duration if args.duration is not None else 30.72
        make_vae = lambda: modules.AutoencoderKL(ddconfig=spec.VAE_DDCONFIG, embed_dim=8,                        # noqa: E731
                                                 scale_factor=0.9227914214134216)
    Ht = _long_latent_h(duration)
    starts, weights = ConsistencyTTA.long_plan(Ht, wh, overlap)
    n = len(starts)
    if Ht <= wh:
        raise SystemExit("--duration %.2f s is one window of %d rows: nothing to fuse" % (duration, Ht))
    B = Bl * n                                             # the plain path's batch: the same U-Net rows
    D = ucfg["cross_attention_dim"]

    def build_pipe():
        v = make_vae()
        p = ConsistencyTTA(unet_config=ucfg, vae=v)
        p.to(dev)
        p.unet.init_random_(seed=0)
        v.init_random_(seed=1)
        return p.eval().requires_grad_(False)
    # one pipe per extent, with the same weights: a module keeps ONE decoder / vocoder handle, re-created for another
    # (H, W), and a captured graph holds the addresses of the handle it was recorded on -- the long path on the plain
    # path's module would free what the plain graph replays
    pipe, pipe_long = build_pipe(), build_pipe()
    vae = pipe.vae
    W_IN = 4.0
    g = torch.Generator(device="cpu").manual_seed(3)
    batches = []
    for _ in range(2):
        lens = torch.randint(min(6, L), L + 1, (B,), generator=g)
        enc, mask = (torch.randn(B, L, D, generator=g) * 0.25).to(dev), (torch.arange(L)[None, :] < lens[:, None]).to(dev)
        batches.append({"enc": enc, "mask": mask, "noise": torch.randn((steps, B, C, wh, W), generator=g).to(dev),
                        "long_enc": enc[:Bl].contiguous(), "long_mask": mask[:Bl].contiguous(),
                        "long_noise": torch.randn((steps, Bl, C, Ht, W), generator=g).to(dev)})
    scratch = torch.empty(4, dtype=torch.float32, device=dev)
    samples = int(16000 * duration)

    def eager_plain(b):
        lat = pipe.generate_latent(b["enc"], b["mask"], b["noise"][0], W_IN, 1.0, steps, step_noise=b["noise"][1:])
        wav = vae.vocode(vae.decode_first_stage(lat))
        pcm = torch.empty(wav.shape, dtype=torch.int16, device=dev)
        N.check(N.lib().ctta_wav_finalize(N.ptr(wav), wav.numel(), N.ptr(scratch), None, N.ptr(pcm), N.stream_ptr()))
        return pcm

    def eager_long(b):
        lat = pipe_long.generate_long_latent(b["long_enc"], b["long_mask"], b["long_noise"][0], W_IN, 1.0, steps,
                                             overlap=overlap, window_h=wh, step_noise=b["long_noise"][1:])
        return pipe_long._decode_long(lat, scratch)[1][:, :samples]

    ref_plain, ref_long = eager_plain(batches[0]).clone(), eager_long(batches[0]).clone()
    torch.cuda.synchronize()
    gen_plain = pipe.capture_graph(B, L, cfg_scale_input=W_IN, cross_attention_dim=D, latent=(C, wh, W), num_steps=steps)
    gen_long = pipe_long.capture_long_graph(Bl, L, duration, cfg_scale_input=W_IN, num_steps=steps, overlap=overlap,
                                            window_h=wh, cross_attention_dim=D, latent_cw=(C, W))
    b0 = batches[0]
    parity = {"plain_graph": bool(torch.equal(gen_plain(b0["enc"], b0["mask"], b0["noise"]), ref_plain)),
              "long_graph": bool(torch.equal(gen_long(b0["long_enc"], b0["long_mask"], b0["long_noise"]), ref_long))}
    if not all(parity.values()):
        raise SystemExit("a captured form differs from its eager counterpart: %s" % parity)

    turn = [0]

    def nxt():
        turn[0] ^= 1
        return batches[turn[0]]

    def plain_call():
        b = nxt()
        return gen_plain(b["enc"], b["mask"], b["noise"])

    def long_call():
        b = nxt()
        return gen_long(b["long_enc"], b["long_mask"], b["long_noise"])
    forms = {"plain_graph": plain_call, "long_graph": long_call, "plain_eager": lambda: eager_plain(nxt()),
             "long_eager": lambda: eager_long(nxt())}
    for fn in forms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    windows = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            windows[k].append((time.perf_counter() - t0) / args.steps * 1e3)
    med = {k: statistics.median(v) for k, v in windows.items()}

    # ---- the step between two queries alone: one launch against the chain it replaces, device time by events
    c, u = (torch.randn(Bl * n, C, wh, W, generator=g).to(dev) for _ in range(2))
    nz = torch.randn(Bl, C, Ht, W, generator=g).to(dev)
    sig = torch.full((Bl,), 0.7, device=dev)
    w = torch.full((Bl,), 2.0, device=dev)
    wdev = weights.to(dev)
    host_starts = (N.c_int32 * n)(*starts)
    n_long = C * Ht * W
    L_ = N.lib()

    def chain(cfg):
        xw = (((1 - 2.0) * u + 2.0 * c) if cfg else c).view(Bl, n, C, wh, W)
        x0 = torch.zeros(Bl, C, Ht, W, device=dev)
        for k, s in enumerate(starts):
            x0[:, :, s:s + wh] += wdev[k].view(1, 1, wh, 1) * xw[:, k]
        z, out = torch.empty_like(x0), torch.empty_like(x0)
        N.check(L_.ctta_heun_add_noise(N.ptr(x0), N.ptr(nz), N.ptr(sig), N.ptr(z), Bl, n_long, N.stream_ptr()))
        N.check(L_.ctta_heun_scale_model_input(N.ptr(z), N.ptr(sig), N.ptr(out), Bl, n_long, N.stream_ptr()))
        cut = torch.stack([out[:, :, s:s + wh] for s in starts], dim=1).reshape(Bl * n, C, wh, W)
        return torch.cat([cut] * 2) if cfg else cut

    def fused(cfg):
        out = torch.empty(((2 if cfg else 1) * Bl * n, C, wh, W), device=dev)
        N.check(L_.ctta_window_fuse_renoise(N.ptr(c), N.ptr(u) if cfg else N.c_void_p(0), N.ptr(w) if cfg else N.c_void_p(0),
                                            host_starts, N.ptr(wdev), N.ptr(nz), N.ptr(sig), N.c_void_p(0), N.ptr(out),
                                            2 if cfg else 1, Bl, n, C, wh, Ht, W, N.stream_ptr()))
        return out
    step_parity = {("cfg" if cfg else "cond"): bool(torch.equal(chain(cfg), fused(cfg))) for cfg in (False, True)}
    step_forms = {"chain_cond": lambda: chain(False), "fused_cond": lambda: fused(False),
                  "chain_cfg": lambda: chain(True), "fused_cfg": lambda: fused(True)}
    step_us = {k: [] for k in step_forms}
    reps = 200
    for _ in range(args.rounds + 1):           # the first round warms up and is dropped
        for k, fn in step_forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            step_us[k].append(e0.elapsed_time(e1) / reps * 1e3)
    step_med = {k: statistics.median(v[1:]) for k, v in step_us.items()}
    result = {
        "tool": "tools/serve_bench.py --long", "device": torch.cuda.get_device_name(0), "tiny": bool(args.tiny),
        "long": {"clips": Bl, "duration_s": duration, "latent_h": Ht, "window_h": wh, "overlap": overlap, "windows": n,
                 "starts": starts, "unet_rows": Bl * n, "decoder_rows_x_latent_h": Bl * Ht, "seconds_of_audio": Bl * duration},
        "plain": {"clips": B, "latent_h": wh, "unet_rows": B, "decoder_rows_x_latent_h": B * wh,
                  "seconds_of_audio": B * wh * 0.04},
        "text_len": L, "num_steps": steps, "steps_per_window": args.steps, "rounds": args.rounds, "warmup_calls": args.warmup,
        "unit": "ms per call of one batch; step kernels: us per step, stream time by events over %d back-to-back steps "
                "(launch cost included)" % reps,
        "timing": "host clock around a window of calls ending in a device synchronise; forms alternate within a round",
        "parity_bit_identical_to_eager": parity, "step_parity_equal": step_parity,
        "ms_per_call_median": {k: round(v, 3) for k, v in med.items()},
        "ms_per_call_windows": {k: [round(x, 3) for x in v] for k, v in windows.items()},
        "ratios_of_medians": {"long_graph_over_plain_graph": round(med["long_graph"] / med["plain_graph"], 4),
                              "long_eager_over_plain_eager": round(med["long_eager"] / med["plain_eager"], 4),
                              "long_graph_over_long_eager": round(med["long_graph"] / med["long_eager"], 4)},
        "step_us_median": {k: round(v, 2) for k, v in step_med.items()},
        "step_us_windows": {k: [round(x, 2) for x in v[1:]] for k, v in step_us.items()},
        "step_fused_over_chain": {"cond": round(step_med["fused_cond"] / step_med["chain_cond"], 4),
                                  "cfg": round(step_med["fused_cfg"] / step_med["chain_cfg"], 4)},
    }
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


def long_edit_leg(args):
    """`--long-edit`: the captured long edit (capture_long_edit_graph: `--long-clips` clips of `--duration` seconds, the
    first `--source-seconds` of each kept from a source latent, the rest generated -- a continuation) beside the captured
    plain long path (capture_long_graph) at the same clips, windows and `--edit-steps` queries, states in, in alternating
    windows; the eager forms of both; and the one-pass step kernel (ctta_window_fuse_edit_renoise) beside the launches it
    replaces (torch combine, slices, torch weighted sum, torch blend, ctta_heun_add_noise, ctta_heun_scale_model_input, the
    cut into windows, torch.cat) and beside ctta_window_fuse_renoise on one long batch.  Both paths run on ONE module: they
    decode the same extent, so they share its decoder and vocoder handles.  The source latent is synthetic: the waveform ->
    latent half runs eagerly before a replay and is not part of either form."""
    import torch
    from consistencytta_amd import _native as N
    from consistencytta_amd import modules, spec
    from consistencytta_amd.models import ConsistencyTTA, _long_latent_h
    dev = "cuda:0"
    Bl, L, steps = args.long_clips, args.text_len, args.edit_steps
    if args.tiny:
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        import cases
        ucfg, (C, wh, W), overlap = dict(cases.TINY_UNET), (8, 32, 16), 8
        duration = args.duration if args.duration is not None else 3.0
        source_s = args.source_seconds if args.source_seconds is not None else 1.0
        vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    else:
        ucfg, (C, wh, W), overlap = spec.LIGHT_UNET_CONFIG, (8, 256, 16), 64
        duration = args.duration if args.duration is not None else 30.72
        source_s = args.source_seconds if args.source_seconds is not None else 10.24
        vae = modules.AutoencoderKL(ddconfig=spec.VAE_DDCONFIG, embed_dim=8, scale_factor=0.9227914214134216)
    Ht = _long_latent_h(duration)
    starts, weights = ConsistencyTTA.long_plan(Ht, wh, overlap)
    n = len(starts)
    if Ht <= wh:
        raise SystemExit("--duration %.2f s is one window of %d rows: nothing to fuse" % (duration, Ht))
    kept_rows = int(source_s * 25) - 2                     # `extend`'s plane for a source at 0 with junction_rows = 2
    if not 0 < kept_rows < Ht:
        raise SystemExit("--source-seconds %.2f does not lie inside the clip" % source_s)
    D = ucfg["cross_attention_dim"]
    pipe = ConsistencyTTA(unet_config=ucfg, vae=vae)
    pipe.to(dev)
    pipe.unet.init_random_(seed=0)
    vae.init_random_(seed=1)
    pipe.eval().requires_grad_(False)
    W_IN = 4.0
    g = torch.Generator(device="cpu").manual_seed(3)
    keep = torch.zeros(1, 1, Ht, W)
    keep[:, :, :kept_rows] = 1
    keep = keep.to(dev)
    batches = []
    for _ in range(2):
        lens = torch.randint(min(6, L), L + 1, (Bl,), generator=g)
        src = torch.randn((Bl, C, Ht, W), generator=g) * 0.8
        src[:, :, kept_rows + 2:] = 0                      # as `extend` builds it: zeros where there is no source
        batches.append({"enc": (torch.randn(Bl, L, D, generator=g) * 0.25).to(dev),
                        "mask": (torch.arange(L)[None, :] < lens[:, None]).to(dev),
                        "noise": torch.randn((steps, Bl, C, Ht, W), generator=g).to(dev), "src": src.to(dev)})
    scratch = torch.empty(4, dtype=torch.float32, device=dev)
    samples = int(16000 * duration)

    def eager_long(b):
        lat = pipe.generate_long_latent(b["enc"], b["mask"], b["noise"][0], W_IN, 1.0, steps, overlap=overlap, window_h=wh,
                                        step_noise=b["noise"][1:])
        return pipe._decode_long(lat, scratch)[1][:, :samples]

    def eager_edit(b):
        lat = pipe.edit_long_latent(b["enc"], b["mask"], b["noise"][0], b["src"], keep, 1.0, W_IN, 1.0, steps,
                                    overlap=overlap, window_h=wh, step_noise=b["noise"][1:])
        return pipe._decode_long(lat, scratch)[1][:, :samples]

    ref_long, ref_edit = eager_long(batches[0]).clone(), eager_edit(batches[0]).clone()
    torch.cuda.synchronize()
    kw0 = dict(cfg_scale_input=W_IN, num_steps=steps, overlap=overlap, window_h=wh, cross_attention_dim=D, latent_cw=(C, W))
    gen_long = pipe.capture_long_graph(Bl, L, duration, **kw0)
    gen_edit = pipe.capture_long_edit_graph(Bl, L, duration, **kw0)
    b0 = batches[0]
    parity = {"long_graph": bool(torch.equal(gen_long(b0["enc"], b0["mask"], b0["noise"]), ref_long)),
              "long_edit_graph": bool(torch.equal(gen_edit(b0["enc"], b0["mask"], b0["noise"], b0["src"], keep), ref_edit))}
    if not all(parity.values()):
        raise SystemExit("a captured form differs from its eager counterpart: %s" % parity)

    turn = [0]

    def nxt():
        turn[0] ^= 1
        return batches[turn[0]]

    def long_call():
        b = nxt()
        return gen_long(b["enc"], b["mask"], b["noise"])

    def edit_call():
        b = nxt()
        return gen_edit(b["enc"], b["mask"], b["noise"], b["src"], keep)
    forms = {"long_graph": long_call, "long_edit_graph": edit_call, "long_eager": lambda: eager_long(nxt()),
             "long_edit_eager": lambda: eager_edit(nxt())}
    for fn in forms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    windows = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            windows[k].append((time.perf_counter() - t0) / args.steps * 1e3)
    med = {k: statistics.median(v) for k, v in windows.items()}

    # ---- the step between two queries alone: one launch against the chain it replaces, device time by events
    c, u = (torch.randn(Bl * n, C, wh, W, generator=g).to(dev) for _ in range(2))
    nz = torch.randn(Bl, C, Ht, W, generator=g).to(dev)
    src = batches[0]["src"]
    sig = torch.full((Bl,), 0.7, device=dev)
    w = torch.full((Bl,), 2.0, device=dev)
    wdev = weights.to(dev)
    keep2 = keep.expand(Bl, 1, Ht, W).reshape(Bl, Ht * W).contiguous()
    keep4 = keep2.view(Bl, 1, Ht, W)
    host_starts = (N.c_int32 * n)(*starts)
    n_long = C * Ht * W
    L_ = N.lib()

    def chain(cfg):
        xw = (((1 - 2.0) * u + 2.0 * c) if cfg else c).view(Bl, n, C, wh, W)
        x0 = torch.zeros(Bl, C, Ht, W, device=dev)
        for k, s in enumerate(starts):
            x0[:, :, s:s + wh] += wdev[k].view(1, 1, wh, 1) * xw[:, k]
        x0 = keep4 * src + (1 - keep4) * x0
        z, out = torch.empty_like(x0), torch.empty_like(x0)
        N.check(L_.ctta_heun_add_noise(N.ptr(x0), N.ptr(nz), N.ptr(sig), N.ptr(z), Bl, n_long, N.stream_ptr()))
        N.check(L_.ctta_heun_scale_model_input(N.ptr(z), N.ptr(sig), N.ptr(out), Bl, n_long, N.stream_ptr()))
        cut = torch.stack([out[:, :, s:s + wh] for s in starts], dim=1).reshape(Bl * n, C, wh, W)
        return torch.cat([cut] * 2) if cfg else cut

    def fused(cfg):
        out = torch.empty(((2 if cfg else 1) * Bl * n, C, wh, W), device=dev)
        N.check(L_.ctta_window_fuse_edit_renoise(N.ptr(c), N.ptr(u) if cfg else N.c_void_p(0),
                                                 N.ptr(w) if cfg else N.c_void_p(0), host_starts, N.ptr(wdev), N.ptr(src),
                                                 N.ptr(keep2), N.ptr(nz), N.ptr(sig), N.c_void_p(0), N.ptr(out),
                                                 2 if cfg else 1, Bl, n, C, wh, Ht, W, N.stream_ptr()))
        return out

    def fused_plain(cfg):
        out = torch.empty(((2 if cfg else 1) * Bl * n, C, wh, W), device=dev)
        N.check(L_.ctta_window_fuse_renoise(N.ptr(c), N.ptr(u) if cfg else N.c_void_p(0), N.ptr(w) if cfg else N.c_void_p(0),
                                            host_starts, N.ptr(wdev), N.ptr(nz), N.ptr(sig), N.c_void_p(0), N.ptr(out),
                                            2 if cfg else 1, Bl, n, C, wh, Ht, W, N.stream_ptr()))
        return out
    step_parity = {("cfg" if cfg else "cond"): bool(torch.equal(chain(cfg), fused(cfg))) for cfg in (False, True)}
    step_forms = {"chain_cond": lambda: chain(False), "fused_cond": lambda: fused(False),
                  "plain_fused_cond": lambda: fused_plain(False), "chain_cfg": lambda: chain(True),
                  "fused_cfg": lambda: fused(True), "plain_fused_cfg": lambda: fused_plain(True)}
    step_us = {k: [] for k in step_forms}
    reps = 200
    for _ in range(args.rounds + 1):           # the first round warms up and is dropped
        for k, fn in step_forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            step_us[k].append(e0.elapsed_time(e1) / reps * 1e3)
    step_med = {k: statistics.median(v[1:]) for k, v in step_us.items()}
    result = {
        "tool": "tools/serve_bench.py --long-edit", "device": torch.cuda.get_device_name(0), "tiny": bool(args.tiny),
        "long": {"clips": Bl, "duration_s": duration, "latent_h": Ht, "window_h": wh, "overlap": overlap, "windows": n,
                 "starts": starts, "unet_rows": Bl * n, "decoder_rows_x_latent_h": Bl * Ht, "seconds_of_audio": Bl * duration},
        "source": {"seconds": source_s, "kept_rows": [0, kept_rows], "junction_rows": 2},
        "text_len": L, "num_steps": steps, "steps_per_window": args.steps, "rounds": args.rounds, "warmup_calls": args.warmup,
        "unit": "ms per call of one batch; step kernels: us per step, stream time by events over %d back-to-back steps "
                "(launch cost included)" % reps,
        "timing": "host clock around a window of calls ending in a device synchronise; forms alternate within a round",
        "parity_bit_identical_to_eager": parity, "step_parity_equal": step_parity,
        "ms_per_call_median": {k: round(v, 3) for k, v in med.items()},
        "ms_per_call_windows": {k: [round(x, 3) for x in v] for k, v in windows.items()},
        "ratios_of_medians": {"long_edit_graph_over_long_graph": round(med["long_edit_graph"] / med["long_graph"], 4),
                              "long_edit_eager_over_long_eager": round(med["long_edit_eager"] / med["long_eager"], 4),
                              "long_edit_graph_over_long_edit_eager": round(med["long_edit_graph"] / med["long_edit_eager"], 4)},
        "step_us_median": {k: round(v, 2) for k, v in step_med.items()},
        "step_us_windows": {k: [round(x, 2) for x in v[1:]] for k, v in step_us.items()},
        "step_fused_over_chain": {"cond": round(step_med["fused_cond"] / step_med["chain_cond"], 4),
                                  "cfg": round(step_med["fused_cfg"] / step_med["chain_cfg"], 4)},
        "step_edit_over_plain_fused": {"cond": round(step_med["fused_cond"] / step_med["plain_fused_cond"], 4),
                                       "cfg": round(step_med["fused_cfg"] / step_med["plain_fused_cfg"], 4)},
    }
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


def seeded_leg(args):
    """`--seeded`: the seeded captures (capture_graph / capture_long_graph with seeded=True: B seeds in, one
    ctta_philox_normal launch at the head of the graph) beside the plain captures fed a device `torch.randn` per call (the
    caller's RNG, then the copy into the static noise buffer), states in, at `--edit-steps` queries, in alternating windows:
    the plain mode's shape (`--batch` clips of the model's own length) and the long leg's (`--long-clips` clips of
    `--duration` seconds).  Then the draw alone, stream time by events: the fill launch, `torch.randn` of the same shape,
    and the upload of the same bytes from pageable and from pinned host memory.  No threshold: the leg records what the fill
    costs against what it replaces."""
    import torch
    from consistencytta_amd import _native as N
    from consistencytta_amd import modules, spec
    from consistencytta_amd.models import ConsistencyTTA, _long_latent_h
    dev = "cuda:0"
    B, Bl, L, steps = args.batch, args.long_clips, args.text_len, args.edit_steps
    if args.tiny:
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        import cases
        ucfg, (C, wh, W), overlap = dict(cases.TINY_UNET), (8, 32, 16), 8
        duration = args.duration if args.duration is not None else 3.0
        make_vae = lambda: modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9,      # noqa: E731
                                                 hifigan_config=cases.TINY_HIFIGAN)
    else:
        ucfg, (C, wh, W), overlap = spec.LIGHT_UNET_CONFIG, (8, 256, 16), 64
        duration = args.duration if args.duration is not None else 30.72
        make_vae = lambda: modules.AutoencoderKL(ddconfig=spec.VAE_DDCONFIG, embed_dim=8,                        # noqa: E731
                                                 scale_factor=0.9227914214134216)
    Ht = _long_latent_h(duration)
    D = ucfg["cross_attention_dim"]

    def build_pipe():
        v = make_vae()
        p = ConsistencyTTA(unet_config=ucfg, vae=v)
        p.to(dev)
        p.unet.init_random_(seed=0)
        v.init_random_(seed=1)
        return p.eval().requires_grad_(False)
    pipe, pipe_long = build_pipe(), build_pipe()           # one module per decoder extent (see long_leg)
    W_IN = 4.0
    g = torch.Generator(device="cpu").manual_seed(3)
    shapes = {"plain": (steps, B, C, wh, W), "long": (steps, Bl, C, Ht, W)}
    batches = []
    for _ in range(2):
        lens = torch.randint(min(6, L), L + 1, (B,), generator=g)
        enc, mask = (torch.randn(B, L, D, generator=g) * 0.25).to(dev), (torch.arange(L)[None, :] < lens[:, None]).to(dev)
        batches.append({"plain": (enc, mask, torch.randint(-2 ** 62, 2 ** 62, (B,), generator=g)),
                        "long": (enc[:Bl].contiguous(), mask[:Bl].contiguous(), torch.randint(-2 ** 62, 2 ** 62, (Bl,), generator=g))})
    kw = {"plain": dict(cfg_scale_input=W_IN, cross_attention_dim=D, latent=(C, wh, W), num_steps=steps),
          "long": dict(cfg_scale_input=W_IN, num_steps=steps, overlap=overlap, window_h=wh, cross_attention_dim=D,
                       latent_cw=(C, W))}
    gens = {("plain", False): pipe.capture_graph(B, L, **kw["plain"]),
            ("plain", True): pipe.capture_graph(B, L, seeded=True, **kw["plain"]),
            ("long", False): pipe_long.capture_long_graph(Bl, L, duration, **kw["long"]),
            ("long", True): pipe_long.capture_long_graph(Bl, L, duration, seeded=True, **kw["long"])}
    noise_of = {"plain": lambda s: pipe.seeded_noise(s, steps, (C, wh, W)),
                "long": lambda s: pipe_long.seeded_noise(s, steps, (C, Ht, W))}
    parity = {}
    for leg in ("plain", "long"):                          # the seeded capture is the plain one fed seeded_noise, bit for bit
        enc, mask, seeds = batches[0][leg]
        want = gens[(leg, False)](enc, mask, noise_of[leg](seeds)).clone()
        parity[leg + "_seeded_graph"] = bool(torch.equal(gens[(leg, True)](enc, mask, seeds), want))
    if not all(parity.values()):
        raise SystemExit("a seeded capture differs from the plain capture fed seeded_noise: %s" % parity)

    turn = [0]

    def nxt(leg):
        turn[0] ^= 1
        return batches[turn[0]][leg]

    def randn_call(leg):
        enc, mask, _ = nxt(leg)
        return gens[(leg, False)](enc, mask, torch.randn(shapes[leg], device=dev))

    def seeded_call(leg):
        return gens[(leg, True)](*nxt(leg))                # host seeds: the upload is B int64
    forms = {"plain_graph_device_randn": lambda: randn_call("plain"), "plain_graph_seeded": lambda: seeded_call("plain"),
             "long_graph_device_randn": lambda: randn_call("long"), "long_graph_seeded": lambda: seeded_call("long")}
    for fn in forms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    windows = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            windows[k].append((time.perf_counter() - t0) / args.steps * 1e3)
    med = {k: statistics.median(v) for k, v in windows.items()}

    # ---- the draw alone: stream time by events over back-to-back calls (launch cost included)
    draw_forms = {}
    for leg, p in (("plain", pipe), ("long", pipe_long)):
        shape = shapes[leg]
        seeds = batches[0][leg][2].to(dev)
        out = torch.empty(shape, device=dev)
        pageable, pinned = torch.randn(shape, generator=g), torch.randn(shape, generator=g).pin_memory()
        draw_forms[leg + "_philox_fill"] = (lambda p=p, seeds=seeds, shape=shape: p.seeded_noise(seeds, shape[0], shape[2:]))
        draw_forms[leg + "_torch_randn"] = (lambda shape=shape: torch.randn(shape, device=dev))
        draw_forms[leg + "_upload_pageable"] = (lambda out=out, src=pageable: out.copy_(src))
        draw_forms[leg + "_upload_pinned"] = (lambda out=out, src=pinned: out.copy_(src, non_blocking=True))
    draw_us = {k: [] for k in draw_forms}
    reps = 50
    for _ in range(args.rounds + 1):           # the first round warms up and is dropped
        for k, fn in draw_forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            draw_us[k].append(e0.elapsed_time(e1) / reps * 1e3)
    draw_med = {k: statistics.median(v[1:]) for k, v in draw_us.items()}
    result = {
        "tool": "tools/serve_bench.py --seeded", "device": torch.cuda.get_device_name(0), "tiny": bool(args.tiny),
        "plain": {"clips": B, "noise_shape": list(shapes["plain"]), "noise_bytes": 4 * int(torch.Size(shapes["plain"]).numel())},
        "long": {"clips": Bl, "duration_s": duration, "latent_h": Ht, "noise_shape": list(shapes["long"]),
                 "noise_bytes": 4 * int(torch.Size(shapes["long"]).numel())},
        "text_len": L, "num_steps": steps, "steps_per_window": args.steps, "rounds": args.rounds, "warmup_calls": args.warmup,
        "unit": "ms per call of one batch; draws: us per call, stream time by events over %d back-to-back calls (launch "
                "cost included)" % reps,
        "timing": "host clock around a window of calls ending in a device synchronise; forms alternate within a round",
        "parity_seeded_graph_bit_identical_to_plain_graph_on_seeded_noise": parity,
        "ms_per_call_median": {k: round(v, 3) for k, v in med.items()},
        "ms_per_call_windows": {k: [round(x, 3) for x in v] for k, v in windows.items()},
        "ratios_of_medians": {leg + "_seeded_over_device_randn":
                              round(med[leg + "_graph_seeded"] / med[leg + "_graph_device_randn"], 4) for leg in ("plain", "long")},
        "draw_us_median": {k: round(v, 2) for k, v in draw_med.items()},
        "draw_us_windows": {k: [round(x, 2) for x in v[1:]] for k, v in draw_us.items()},
    }
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


def adapters_leg(args):
    """`--adapters`: what a batch costs when its rows ask for different LoRA adapters.  Light U-Net (`--tiny`: the tiny one),
    `--batch` clips, rank 4, four adapters, one query, states in, every form one captured hipGraph of the whole pipeline, in
    alternating windows:

      (a) plain            no adapters at all
      (b) single_adapter   one adapter for all rows on the single-adapter path (the module's own adapters)
      (c) mixed_rows       capture_graph(adapters=True): a quarter of the rows per adapter, looked up per row
      (d) split_and_swap   what a server does without (c): four quarter-batch single-adapter replays with an adapter-only
                           reload (ctta_unet_load_adapters) in front of each

    (c) / (b) is the price of the per-row lookup, (c) / (d) what mixing buys.  Checked before anything is timed: (c) with one
    adapter in every row gives the latent of (b) bit for bit.  No threshold: the leg records."""
    import torch
    from collections import OrderedDict
    from consistencytta_amd import _native as N
    from consistencytta_amd import modules, spec
    from consistencytta_amd.models import ConsistencyTTA
    dev = "cuda:0"
    B, L, RANK, NA = args.batch, args.text_len, 4, 4
    if B % NA:
        raise SystemExit("--batch must be a multiple of %d" % NA)
    Bq = B // NA
    if args.tiny:
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        import cases
        ucfg, latent = dict(cases.TINY_UNET), (8, 32, 16)
        make_vae = lambda: modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9,      # noqa: E731
                                                 hifigan_config=cases.TINY_HIFIGAN)
    else:
        ucfg, latent = spec.LIGHT_UNET_CONFIG, (8, 256, 16)
        make_vae = lambda: modules.AutoencoderKL(ddconfig=spec.VAE_DDCONFIG, embed_dim=8,                        # noqa: E731
                                                 scale_factor=0.9227914214134216)
    D = ucfg["cross_attention_dim"]
    g = torch.Generator(device="cpu").manual_seed(5)
    sets = []
    for _ in range(NA):          # down as LoRALinearLayer's init (std 1 / rank), up small but non-zero
        sets.append(OrderedDict((k, torch.randn(shape, generator=g) * (1.0 / RANK if k.endswith("down.weight") else 0.02))
                                for k, shape in spec.lora_param_spec(ucfg, RANK).items()))

    def build_pipe(lora):
        v = make_vae()
        p = ConsistencyTTA(unet_config=ucfg, vae=v)
        p.to(dev)
        p.unet.init_random_(seed=0)
        v.init_random_(seed=1)
        if lora:
            p.unet.enable_lora_(RANK)
            p.unet.load_state_dict(sets[0], strict=False)
        return p.eval().requires_grad_(False)
    plain, single, bank, swap = build_pipe(False), build_pipe(True), build_pipe(True), build_pipe(True)
    names = ["style%d" % i for i in range(NA)]
    for n, sd in zip(names, sets):
        bank.unet.add_adapter(n, sd)
    W_IN = 4.0
    batches = []
    for _ in range(2):
        lens = torch.randint(min(6, L), L + 1, (B,), generator=g)
        batches.append(((torch.randn(B, L, D, generator=g) * 0.25).to(dev), (torch.arange(L)[None, :] < lens[:, None]).to(dev),
                        torch.randn((B,) + latent, generator=g).to(dev)))
    kw = dict(cfg_scale_input=W_IN, cross_attention_dim=D, latent=latent, num_steps=1)
    g_plain, g_single = plain.capture_graph(B, L, **kw), single.capture_graph(B, L, **kw)
    g_mixed = bank.capture_graph(B, L, adapters=True, **kw)
    g_swap = swap.capture_graph(Bq, L, **kw)
    mixed_rows = [names[i // Bq] for i in range(B)]
    # (d) in its cheapest form: the four sets are device resident, a swap is ONE multi-tensor copy into the module's adapter
    # parameters and ONE ctta_unet_load_adapters from them (the same source pointers every time: no job table is uploaded)
    own = OrderedDict((k, p.data) for k, p in swap.unet.named_parameters() if "_lora." in k)
    own_table, _keep = N.tensor_table(own)
    dev_sets = [[sd[k].to(dev) for k in own] for sd in sets]
    swap_h = swap.unet._h_unet

    def swap_call(enc, mask, noise):
        out = None
        for i, srcs in enumerate(dev_sets):
            torch._foreach_copy_(list(own.values()), srcs)
            N.check(N.lib().ctta_unet_load_adapters(swap_h, own_table, len(own_table), N.stream_ptr()))
            out = g_swap(enc[i * Bq:(i + 1) * Bq], mask[i * Bq:(i + 1) * Bq], noise[i * Bq:(i + 1) * Bq])
        return out

    enc, mask, noise = batches[0]
    g_single(enc, mask, noise)
    want = g_single.outputs[0].clone()
    g_mixed(enc, mask, noise, adapters=[names[0]] * B)
    parity = {"mixed_rows_all_one_adapter_equals_single_adapter": bool(torch.equal(g_mixed.outputs[0], want))}
    g_mixed(enc, mask, noise, adapters=mixed_rows)
    parity["mixed_rows_differ_from_single_adapter"] = not bool(torch.equal(g_mixed.outputs[0], want))
    swap_call(enc, mask, noise)
    last = g_swap.outputs[0].clone()
    parity["swap_last_quarter_differs_from_adapter_0"] = not bool(torch.equal(last, want[:Bq]))
    if not all(parity.values()):
        raise SystemExit("the adapter forms disagree: %s" % parity)

    turn = [0]

    def nxt():
        turn[0] ^= 1
        return batches[turn[0]]
    forms = {"plain": lambda: g_plain(*nxt()), "single_adapter": lambda: g_single(*nxt()),
             "mixed_rows": lambda: g_mixed(*nxt(), adapters=mixed_rows), "split_and_swap": lambda: swap_call(*nxt())}
    for fn in forms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    windows = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            windows[k].append((time.perf_counter() - t0) / args.steps * 1e3)
    med = {k: statistics.median(v) for k, v in windows.items()}
    result = {
        "tool": "tools/serve_bench.py --adapters", "device": torch.cuda.get_device_name(0), "tiny": bool(args.tiny),
        "clips_per_call": B, "adapters": NA, "rows_per_adapter": Bq, "rank": RANK, "text_len": L, "num_steps": 1,
        "latent": list(latent), "steps_per_window": args.steps, "rounds": args.rounds, "warmup_calls": args.warmup,
        "unit": "ms per call of one batch of %d clips (split_and_swap: %d reloads + %d replays of %d clips)" % (B, NA, NA, Bq),
        "timing": "host clock around a window of calls ending in a device synchronise; forms alternate within a round",
        "parity": parity,
        "ms_per_call_median": {k: round(v, 3) for k, v in med.items()},
        "clips_per_s_median": {k: round(B / v * 1e3, 1) for k, v in med.items()},
        "ms_per_call_windows": {k: [round(x, 3) for x in v] for k, v in windows.items()},
        "ratios_of_medians": {"single_over_plain": round(med["single_adapter"] / med["plain"], 4),
                              "mixed_over_single": round(med["mixed_rows"] / med["single_adapter"], 4),
                              "mixed_over_split_and_swap": round(med["mixed_rows"] / med["split_and_swap"], 4)},
    }
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--adapters", action="store_true", help="only the adapter leg: a batch with a different LoRA adapter per "
                    "row beside the plain, the single-adapter and the split-and-swap forms")
    ap.add_argument("--seeded", action="store_true", help="only the seeded leg: the seeded captures beside the plain captures "
                    "fed a device torch.randn per call, and the fill launch beside the draws and uploads it replaces")
    ap.add_argument("--long", action="store_true", help="only the long-clip leg: the captured long path beside the captured "
                    "plain few-step path at the same number of U-Net rows, and the one-pass step kernel beside its chain")
    ap.add_argument("--long-edit", action="store_true", help="only the long-edit leg: the captured long edit beside the "
                    "captured plain long path, and the one-pass edit step kernel beside the chain it replaces")
    ap.add_argument("--source-seconds", type=float, default=None, help="seconds of source kept at the start of every clip of "
                    "the long-edit leg (default 10.24; --tiny: 1.0)")
    ap.add_argument("--duration", type=float, default=None, help="seconds per clip of the long leg (default 30.72; --tiny: 3.0)")
    ap.add_argument("--long-clips", type=int, default=8, help="clips per call of the long leg")
    ap.add_argument("--edit", action="store_true", help="only the editing leg: the captured edit path beside the captured "
                    "plain few-step path, and the one-pass step kernel beside the chain it replaces")
    ap.add_argument("--edit-steps", type=int, default=4, help="num_steps of the editing leg")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--text-len", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=4, help="calls per form before the first window")
    ap.add_argument("--rounds", type=int, default=5, help="windows per form, alternating the forms")
    ap.add_argument("--tiny", action="store_true", help="tiny networks (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from consistencytta_amd import _native as N
    from consistencytta_amd import modules, spec, text_encoder
    from consistencytta_amd.models import ConsistencyTTA
    if not torch.cuda.is_available():
        raise SystemExit("serve_bench needs a GPU: there is no CPU path and no number without one")
    if args.adapters:
        return adapters_leg(args)
    if args.edit:
        return edit_leg(args)
    if args.long:
        return long_leg(args)
    if args.long_edit:
        return long_edit_leg(args)
    if args.seeded:
        return seeded_leg(args)
    dev = "cuda:0"
    B, L = args.batch, args.text_len

    if args.tiny:
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        import cases
        t5_cfg = cases.TINY_T5
        ucfg = dict(cases.TINY_UNET, cross_attention_dim=t5_cfg["d_model"])
        vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
        latent = (8, 32, 16)
    else:
        t5_cfg, ucfg, latent = spec.T5_LARGE_CONFIG, spec.LIGHT_UNET_CONFIG, (8, 256, 16)
        vae = modules.AutoencoderKL(ddconfig=spec.VAE_DDCONFIG, embed_dim=8, scale_factor=0.9227914214134216)
    D = ucfg["cross_attention_dim"]
    te = text_encoder.T5EncoderModel(t5_cfg)
    pipe = ConsistencyTTA(unet_config=ucfg, vae=vae, text_encoder=te)
    pipe.to(dev)
    pipe.unet.init_random_(seed=0)
    vae.init_random_(seed=1)
    te.init_random_(seed=7)
    pipe.eval().requires_grad_(False)

    # ---- synthetic AudioCaps-shaped inputs: two different batches of host tokens with ragged masks, device-resident draws
    g = torch.Generator(device="cpu").manual_seed(3)
    batches = []
    for _ in range(2):
        ids = torch.randint(2, t5_cfg["vocab_size"], (B, L), generator=g)
        lens = torch.randint(min(6, L), L + 1, (B,), generator=g)
        am = (torch.arange(L)[None, :] < lens[:, None]).to(torch.int64)
        ids = ids * am
        noise = torch.randn((2, B) + latent, generator=g).to(dev)     # row 0 the initial draw, row 1 the step noise
        batches.append({"ids": ids, "am": am, "noise": noise})
    unc_ids = torch.zeros(B, L, dtype=torch.int64)
    unc_ids[:, 0] = 1                                                  # the prompt "": EOS, then padding
    unc_am = torch.zeros(B, L, dtype=torch.int64)
    unc_am[:, 0] = 1
    W_IN, W_POST = 4.0, 2.0
    scratch = torch.empty(4, dtype=torch.float32, device=dev)

    def encode(ids, am):
        """`encode_text` from ready tokens: upload, T5EncoderModel.forward (with its range checks), bool mask."""
        ids, am = ids.to(dev), am.to(dev)
        return te(input_ids=ids, attention_mask=am)[0], am == 1

    unc, unc_mask = encode(unc_ids, unc_am)
    for b in batches:
        b["enc"], b["mask"] = encode(b["ids"], b["am"])

    def eager(b, steps, post):
        kw = dict(uncond_states=unc, uncond_mask=unc_mask) if post > 1 else {}
        lat = pipe.generate_latent(b["enc"], b["mask"], b["noise"][0], W_IN, post, steps, step_noise=b["noise"][1:steps], **kw)
        wav = vae.vocode(vae.decode_first_stage(lat))
        pcm = torch.empty(wav.shape, dtype=torch.int16, device=dev)
        N.check(N.lib().ctta_wav_finalize(N.ptr(wav), wav.numel(), N.ptr(scratch), None, N.ptr(pcm), N.stream_ptr()))
        return pcm

    # every handle at its final size BEFORE the first capture: a captured graph holds the addresses of the handle it was
    # recorded on, and a later call that needs a bigger one (post-CFG: 2B rows) would replace it
    ref = {(s, p): [eager(b, s, p).clone() for b in batches] for s, p in ((2, W_POST), (2, 1.0), (1, 1.0))}
    torch.cuda.synchronize()

    kw0 = dict(cfg_scale_input=W_IN, cross_attention_dim=D, latent=latent)
    few = {"steps2": dict(num_steps=2), "steps2_post2": dict(num_steps=2, cfg_scale_post=W_POST, uncond_states=unc,
                                                            uncond_mask=unc_mask)}
    gen_a = pipe.capture_pipeline(B, L, **kw0)
    gen_c = pipe.capture_pipeline(B, L, from_tokens=True, **kw0)
    gen_g = {k: pipe.capture_graph(B, L, **kw0, **v) for k, v in few.items()}
    gen_p = {k: pipe.capture_pipeline(B, L, **kw0, **v) for k, v in few.items()}
    placement = {"states_pipeline": gen_a.placement_ms, "tokens_pipeline": gen_c.placement_ms}
    placement.update({k + "_pipeline": v.placement_ms for k, v in gen_p.items()})

    def feed(fn, depth, arg):
        """What a pipeline returns for batch 0 followed by batch 1 `depth` times: batch 0's result."""
        fn(*arg(batches[0]))
        for _ in range(depth):
            out = fn(*arg(batches[1]))
        return out.clone()

    a_args = lambda b: (b["enc"], b["mask"], b["noise"][0])                                     # noqa: E731
    c_args = lambda b: (b["ids"], b["am"], b["noise"][0])                                       # noqa: E731
    f_args = lambda b: (b["enc"], b["mask"], b["noise"])                                        # noqa: E731

    def form_b(b):
        enc, mask = encode(b["ids"], b["am"])
        return gen_a(enc, mask, b["noise"][0])

    parity = {"states_pipeline": bool(torch.equal(feed(gen_a, 2, a_args), ref[(1, 1.0)][0])),
              "tokens_pipeline": bool(torch.equal(feed(gen_c, 3, c_args), ref[(1, 1.0)][0]))}
    for k, v in few.items():
        key = (2, v.get("cfg_scale_post", 1.0))
        parity[k + "_graph"] = bool(torch.equal(gen_g[k](*f_args(batches[0])), ref[key][0]))
        parity[k + "_pipeline"] = bool(torch.equal(feed(gen_p[k], 2, f_args), ref[key][0]))
    if not all(parity.values()):
        raise SystemExit("a captured form differs from its eager counterpart: %s" % parity)

    turn = [0]

    def nxt():
        turn[0] ^= 1
        return batches[turn[0]]
    forms = {"states_pipeline": lambda: gen_a(*a_args(nxt())),
             "eager_t5_then_pipeline": lambda: form_b(nxt()),
             "tokens_pipeline": lambda: gen_c(*c_args(nxt()))}
    for k, v in few.items():
        s, p = 2, v.get("cfg_scale_post", 1.0)
        forms[k + "_eager"] = (lambda s=s, p=p: eager(nxt(), s, p))
        forms[k + "_graph"] = (lambda k=k: gen_g[k](*f_args(nxt())))
        forms[k + "_pipeline"] = (lambda k=k: gen_p[k](*f_args(nxt())))

    for fn in forms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    windows = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            windows[k].append((time.perf_counter() - t0) / args.steps * 1e3)
    med = {k: statistics.median(v) for k, v in windows.items()}
    ratios = {"c_over_b": med["tokens_pipeline"] / med["eager_t5_then_pipeline"],
              "c_over_a": med["tokens_pipeline"] / med["states_pipeline"],
              "b_over_a": med["eager_t5_then_pipeline"] / med["states_pipeline"]}
    for k in few:
        ratios[k + "_graph_over_eager"] = med[k + "_graph"] / med[k + "_eager"]
        ratios[k + "_pipeline_over_eager"] = med[k + "_pipeline"] / med[k + "_eager"]
    result = {
        "tool": "tools/serve_bench.py", "device": torch.cuda.get_device_name(0), "tiny": bool(args.tiny),
        "batch": B, "text_len": L, "latent": list(latent), "steps_per_window": args.steps, "rounds": args.rounds,
        "warmup_calls": args.warmup, "unit": "ms per call (one batch enters and one leaves per call)",
        "timing": "host clock around a window of calls ending in a device synchronise; forms alternate within a round",
        "parity_bit_identical_to_eager": parity,
        "ms_per_call_median": {k: round(v, 3) for k, v in med.items()},
        "ms_per_call_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in windows.items()},
        "ms_per_call_windows": {k: [round(x, 3) for x in v] for k, v in windows.items()},
        "clips_per_s_median": {k: round(B / v * 1e3, 2) for k, v in med.items()},
        "ratios_of_medians": {k: round(v, 4) for k, v in ratios.items()},
        "placement_ms": placement,
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
