"""The long-clip sampler of `ConsistencyTTA.generate_long_latent` restated as plain fp32 torch around a `query(z_in, t)`
callable (the guided student with its post-CFG combine on B * n window rows, row b * n + k: scaled input in, x0 estimate
out).  What it restates:

  the few-step sampler     easy_inference/consistencytta.py:152-197, through edit_ref.schedule / add_noise / scale_model_input
  the clip's extent        audioldm/pipeline.py:49-50,94-95 (duration -> latent rows); here the rows are given
  the window plan          evenly spread starts with integer round-half-up, ramp weights over the overlaps normalised in
                           float64 so that every long row's weights sum to 1 -- from the formulas, not from `long_plan`
  the fusion               x0_long[h] = sum over the covering windows k, ascending, of weights[k][h - starts[k]] * x0_k
                           (the first term assigned, the others added), between two queries and at the end
  the step                 ONE long draw per step: add_noise and scale_model_input on the long x0, then the cut into windows

Every operation is its own torch kernel, so nothing is contracted."""
import numpy as np
import torch

import edit_ref


def plan(latent_h, window_h, overlap):
    """(starts, weights (n, rows) fp32) of a latent of `latent_h` rows under windows of `window_h` rows."""
    if latent_h <= window_h:
        return [0], torch.ones(1, latent_h)
    span = latent_h - window_h
    step = window_h - overlap
    n = (span + step - 1) // step + 1
    starts = [(2 * k * span + (n - 1)) // (2 * (n - 1)) for k in range(n)]
    raw = []
    for k in range(n):
        ovl = starts[k - 1] + window_h - starts[k] if k else 0
        ovr = starts[k] + window_h - starts[k + 1] if k < n - 1 else 0
        raw.append([min(1.0, (j + 1) / (ovl + 1)) * min(1.0, (window_h - j) / (ovr + 1)) for j in range(window_h)])
    total = [0.0] * latent_h
    for k in range(n):
        for j in range(window_h):
            total[starts[k] + j] += raw[k][j]
    w = np.array([[raw[k][j] / total[starts[k] + j] for j in range(window_h)] for k in range(n)], dtype=np.float64)
    return starts, torch.from_numpy(w.astype(np.float32))


def cut(long, starts, rows):
    """(B, C, Ht, W) -> (B * n, C, rows, W), row b * n + k."""
    B = long.shape[0]
    wins = torch.stack([long[:, :, s:s + rows] for s in starts], dim=1)
    return wins.reshape((B * len(starts),) + tuple(wins.shape[2:])).contiguous()


def fuse(x0_windows, starts, weights, latent_h):
    """(B * n, C, rows, W) -> (B, C, latent_h, W): the weighted overlap-add, windows in ascending order; the first window
    over a row assigns its term, the others add theirs."""
    n, rows = weights.shape
    Bn, C, _, W = x0_windows.shape
    x = x0_windows.reshape(Bn // n, n, C, rows, W)
    wt = weights.to(x.device)
    acc = torch.zeros(Bn // n, C, latent_h, W, dtype=torch.float32, device=x.device)
    seen = torch.zeros(latent_h, dtype=torch.bool, device=x.device)
    for k, s in enumerate(starts):
        term = wt[k].view(1, 1, rows, 1) * x[:, k]
        added = acc[:, :, s:s + rows] + term
        acc[:, :, s:s + rows] = torch.where(seen[s:s + rows].view(1, 1, rows, 1), added, term)
        seen[s:s + rows] = True
    assert bool(seen.all())
    return acc


def long_sampler(query, times, sigmas, noise, window_h, overlap, step_noise=()):
    """`times` / `sigmas`: edit_ref.schedule; `noise`: (B, C, Ht, W); `step_noise`: len(times) - 1 long draws."""
    Ht = noise.shape[2]
    starts, weights = plan(Ht, window_h, overlap)
    rows = weights.shape[1]
    draws = [noise] + list(step_noise)
    assert len(draws) == len(times)
    x0 = torch.zeros_like(noise)
    for k in range(len(times)):
        z = edit_ref.scale_model_input(edit_ref.add_noise(x0, draws[k], sigmas[k]), sigmas[k])
        x0 = fuse(query(cut(z, starts, rows), times[k]), starts, weights, Ht)
    return x0
