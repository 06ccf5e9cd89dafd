"""The long-clip edit sampler of `ConsistencyTTA.edit_long_latent` restated as plain fp32 torch around a `query(z_in, t)`
callable (the guided student with its post-CFG combine on B * n window rows, row b * n + k: scaled input in, x0 estimate
out).  It is tests/long_ref.py with the source of tests/edit_ref.py:

  the window plan, the cut, the fusion     long_ref.plan / cut / fuse
  the query times, add_noise, scaling      edit_ref.schedule / add_noise / scale_model_input
  the blend                                audioldm/latent_diffusion/ddim.py:216, img_orig * mask + (1 - mask) * img, on the
                                           FUSED long x0 after every query, under a (B or 1, 1, Ht, W) mask
  how many queries run                     audioldm/pipeline.py:216: the LAST r = max(1, int(strength * num_steps)) times;
                                           r == num_steps starts from the blend of x0 = 0, r < num_steps from the source

Every operation is its own torch kernel, so nothing is contracted."""
import torch

import edit_ref
import long_ref


def blend(x0, src, keep):
    """keep * src + (1 - keep) * x0; `keep` None keeps nothing and leaves x0 as it is."""
    return x0 if keep is None else keep * src + (1 - keep) * x0


def long_edit_sampler(query, times, sigmas, noise, src, keep, window_h, overlap, strength=1.0, step_noise=()):
    """`times` / `sigmas`: all num_steps query times (edit_ref.schedule); `noise`, `src`: (B, C, Ht, W); `keep`:
    broadcastable to `src` or None; `step_noise`: r - 1 long draws."""
    num_steps = len(times)
    r = max(1, int(strength * num_steps))
    times, sigmas = times[num_steps - r:], sigmas[num_steps - r:]
    Ht = noise.shape[2]
    starts, weights = long_ref.plan(Ht, window_h, overlap)
    rows = weights.shape[1]
    draws = [noise] + list(step_noise)
    assert len(draws) == r
    x0 = blend(torch.zeros_like(src), src, keep) if r == num_steps else src
    for k in range(r):
        z = edit_ref.scale_model_input(edit_ref.add_noise(x0, draws[k], sigmas[k]), sigmas[k])
        x0 = blend(long_ref.fuse(query(long_ref.cut(z, starts, rows), times[k]), starts, weights, Ht), src, keep)
    return x0
