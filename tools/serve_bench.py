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


def main():
    ap = argparse.ArgumentParser()
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
