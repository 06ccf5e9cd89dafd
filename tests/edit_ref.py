"""The edit sampler of `ConsistencyTTA.edit_latent` restated as plain fp32 torch around a `query(z_in, t)` callable (the
guided student with its post-CFG combine: scaled input in, x0 estimate out).  What it restates:

  the few-step sampler     easy_inference/consistencytta.py:152-197 (first query at the head of the 18-step table, the others
                           at set_timesteps(num_steps).timesteps[1::2], re-noised from x0 before each)
  add_noise                scheduling_heun_discrete.py:384          x0 + noise * sigma
  scale_model_input        scheduling_heun_discrete.py:170-171      z / (sigma ** 2 + 1) ** 0.5
  the blend                audioldm/latent_diffusion/ddim.py:216    img_orig * mask + (1 - mask) * img, on x0 after every query
  how many queries run     audioldm/pipeline.py:216                 t_enc = int(transfer_strength * ddim_steps): the LAST
                           r = max(1, int(strength * num_steps)) query times

Every operation is its own torch kernel, so nothing is contracted; sigma and the divisor are tensors on the sample's device
(a Python scalar divisor would be turned into a multiplication by its reciprocal)."""
import numpy as np
import torch


def schedule(sch, num_steps):
    """(times, sigmas) of the num_steps queries of `generate_latent`, from the scheduler's host tables: the head of the
    18-step table, then timesteps[1::2] of the num_steps table with the sigma at the LAST index of each time
    (index_for_timestep, scheduling_heun_discrete.py:145-149)."""
    sch.set_timesteps(18)
    times, sigmas = [float(sch._timesteps_host[0])], [np.float32(sch._sigmas_host[0])]
    sch.set_timesteps(num_steps)
    for t in sch._timesteps_host[1::2]:
        idx = int(np.nonzero(sch._timesteps_host == t)[0][-1])
        times.append(float(t))
        sigmas.append(np.float32(sch._sigmas_host[idx]))
    assert len(times) == num_steps
    return times, sigmas


def _rows(value, like):
    return torch.full((like.shape[0], 1, 1, 1), float(value), dtype=torch.float32, device=like.device)


def add_noise(x0, noise, sigma):
    return x0 + noise * _rows(sigma, x0)


def scale_model_input(z, sigma):
    s = np.float32(sigma)
    return z / _rows(np.sqrt(s * s + np.float32(1.0)), z)


def plain_sampler(query, times, sigmas, noise, step_noise=()):
    """consistencytta.py:152-197 on explicit draws."""
    x0 = query(scale_model_input(noise * _rows(sigmas[0], noise), sigmas[0]), times[0])
    for k in range(1, len(times)):
        x0 = query(scale_model_input(add_noise(x0, step_noise[k - 1], sigmas[k]), sigmas[k]), times[k])
    return x0


def edit_sampler(query, times, sigmas, noise, src, keep=None, strength=1.0, step_noise=()):
    """`times` / `sigmas`: all num_steps query times (`schedule`); `keep`: broadcastable to `src`, None keeps nothing;
    `step_noise`: r - 1 draws."""
    num_steps = len(times)
    r = max(1, int(strength * num_steps))
    times, sigmas = times[num_steps - r:], sigmas[num_steps - r:]
    draws = [noise] + list(step_noise)
    assert len(draws) == r

    def blend(x0):
        return x0 if keep is None else keep * src + (1 - keep) * x0

    x0 = blend(torch.zeros_like(src)) if r == num_steps else src
    for k in range(r):
        x0 = blend(query(scale_model_input(add_noise(x0, draws[k], sigmas[k]), sigmas[k]), times[k]))
    return x0
