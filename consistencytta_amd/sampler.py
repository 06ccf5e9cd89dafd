"""Host code of the few-step consistency sampler (easy_inference/consistencytta.py:152-197) behind `ConsistencyTTA`'s plain,
editing and long-clip entries: ONE query loop (`sample`) over three step forms.  A form says how the first U-Net input is
made, which launch turns a query's output into the next query's input, and which launch ends the loop:

| form       | start                                             | between two queries           | end                         |
|------------|---------------------------------------------------|-------------------------------|-----------------------------|
| `Plain`    | torch: noise * init_noise_sigma, cat, scale       | ctta_consistency_renoise      | ctta_cfg_combine (post-CFG) |
| `Keep`     | ctta_consistency_edit_renoise / ..._renoise       | ctta_consistency_edit_renoise | ctta_cfg_combine_keep       |
| `Windows`  | ctta_window_fuse_renoise / ..._edit_renoise       | the same entry                | the same entry -> x0_long   |

Every launch is the same fp32 arithmetic per element as the eager torch sequence it replaces, so the forms are bit-identical
to `generate_latent` and to each other where they meet (one window of the model's height, a zero keep plane)."""
import numpy as np
import torch

from . import _native as N


def _check_step_noise(step_noise, count, noise):
    """`step_noise=` of the few-step samplers: (count, *noise.shape), one re-noising draw per sampler step after the first
    query.  Raises before anything is launched."""
    if step_noise is None:
        return
    want = (int(count),) + tuple(noise.shape)
    if not torch.is_tensor(step_noise) or tuple(step_noise.shape) != want:
        got = tuple(step_noise.shape) if torch.is_tensor(step_noise) else type(step_noise).__name__
        raise ValueError("step_noise %s: expected %s (one draw per re-noising step)" % (got, want))


def _check_edit_inputs(noise, src_latent, keep_mask, strength, num_steps):
    """The host-side rules of `ConsistencyTTA.edit_latent`, raised before anything is launched (they hold on host tensors):
    `noise` is (B, C, H, W), or (r, B, C, H, W) in the captured form, the source has the sample's shape, the mask is
    (B, 1, H, W) or (1, 1, H, W), `strength` lies in (0, 1].  Returns r = max(1, int(strength * num_steps)), the number of
    queries that run (audioldm/pipeline.py:216, t_enc = int(transfer_strength * ddim_steps))."""
    num_steps = int(num_steps)
    if num_steps < 1:
        raise ValueError("num_steps must be at least 1, got %d" % num_steps)
    if not 0. < float(strength) <= 1.:
        raise ValueError("strength %r: expected a number in (0, 1]" % (strength,))
    sample = tuple(noise.shape[-4:])
    if not torch.is_tensor(src_latent) or len(sample) != 4 or tuple(src_latent.shape) != sample:
        got = tuple(src_latent.shape) if torch.is_tensor(src_latent) else type(src_latent).__name__
        raise ValueError("src_latent %s: expected the noise's shape %s" % (got, sample))
    B, _, H, W = sample
    if keep_mask is not None and (not torch.is_tensor(keep_mask) or tuple(keep_mask.shape) not in ((B, 1, H, W), (1, 1, H, W))):
        got = tuple(keep_mask.shape) if torch.is_tensor(keep_mask) else type(keep_mask).__name__
        raise ValueError("keep_mask %s: expected (%d, 1, %d, %d) or (1, 1, %d, %d)" % (got, B, H, W, H, W))
    return max(1, int(float(strength) * num_steps))


def _edit_queries(strength, num_steps):
    """r of `_check_edit_inputs` from the strength / num_steps rules alone: r queries take r draws."""
    shape = torch.empty(1, 0, 1, 1)
    return _check_edit_inputs(shape, shape, None, strength, num_steps)


def _post_cfg_fusable(w):
    """Whether the kernels' post-CFG combine (ctta_consistency_renoise, ctta_cfg_combine: a = 1 - w subtracted in fp32) gives
    torch's `(1 - w) * u + w * c` bit for bit: torch rounds the Python double 1 - w to fp32, so the two coefficients are the
    same number whenever 1 - w is exact in fp32 (every dyadic scale: 1.5, 2, 2.5, 3 ...).  Any other scale keeps torch's own
    combine inside the captured sequence."""
    return bool(np.float32(1.0 - float(w)) == np.float32(1.0) - np.float32(w))


def _cfg_rows(zh, rows, w_post):
    """A query's output -> (cond, uncond) as the step kernels take them.  With post-CFG `zh` holds `rows` uncond rows, then
    `rows` cond rows: the kernel combines them, unless it cannot reproduce the scale bit for bit (`_post_cfg_fusable`);
    then torch combines first and the kernel sees cond rows only.  `zh` None (a sampler's start, x0 = 0): (None, None)."""
    if zh is None:
        return None, None
    if not w_post > 1.:
        return zh, None
    if _post_cfg_fusable(w_post):
        return zh[rows:], zh[:rows]
    return (1 - w_post) * zh[:rows] + w_post * zh[rows:], None


def query_times(sch, num_steps, device, r=None, at_head=None):
    """The query times of the few-step sampler: the head of the 18-step table, then `_timesteps_host[1::2]` of the
    `num_steps` table, cut to the last `r` (None: all).  `at_head(t_head)` runs while the scheduler still holds the 18-step
    table -- the head's sigma and `init_noise_sigma` are read from it; the `num_steps` table of a one-step sampler does not
    hold them.  The scheduler is left in the `num_steps` state.  Returns (times, what `at_head` returned)."""
    sch.set_timesteps(18, device=device)
    t_head = float(sch._timesteps_host[0])
    head = None if at_head is None else at_head(t_head)
    sch.set_timesteps(num_steps, device=device)
    times = [t_head] + [float(v) for v in sch._timesteps_host[1::2]]
    return (times if r is None else times[len(times) - r:]), head


def _keep_plane(keep_mask, B, H, W, dev):
    """The keep mask as the step kernels read it: (B, 1, H, W), (1, 1, H, W) or None (keeps nothing) -> contiguous
    (B, H * W) fp32."""
    if keep_mask is None:
        return torch.zeros(B, H * W, dtype=torch.float32, device=dev)
    return keep_mask.detach().to(dev, torch.float32).expand(B, 1, H, W).reshape(B, H * W).contiguous()


def _window_rows(states, B, n, what):
    """Text states / masks of the long-clip sampler as B * n rows, row b * n + k: B rows are repeated per window, B * n rows
    give every window its own."""
    if states is None or states.shape[0] not in (B, B * n):
        got = None if states is None else tuple(states.shape)
        raise ValueError("%s %s: expected %d rows (repeated per window) or %d (one per window)" % (what, got, B, B * n))
    return states.repeat_interleave(n, 0) if states.shape[0] == B and n > 1 else states


def stack_text(states, mask, uncond_states, uncond_mask, w_post, windows=None):
    """Text states and mask as the queries take them: with post-CFG the uncond rows stand first.  `windows`: (B, n) of the
    long-clip sampler, every tensor then passes `_window_rows`."""
    if windows is not None:
        states, mask = _window_rows(states, *windows, "encoder_states"), _window_rows(mask, *windows, "encoder_mask")
    if not w_post > 1.:
        return states, mask
    if windows is not None:
        uncond_states = _window_rows(uncond_states, *windows, "uncond_states")
        uncond_mask = _window_rows(uncond_mask, *windows, "uncond_mask")
    return torch.cat([uncond_states, states]), torch.cat([uncond_mask, mask])


def draws(noise, step_noise):
    """`draw(k)` of the eager entries: the first noise, then `step_noise[k - 1]`, or a fresh `torch.randn_like` per step
    when none is given, as the reference draws it."""
    def draw(k):
        if k == 0:
            return noise
        return torch.randn_like(noise) if step_noise is None else step_noise[k - 1]
    return draw


def _once(cache, key, make):
    if key not in cache:
        cache[key] = make()
    return cache[key]


class Plain:
    """The sampler of `generate_latent` in the form the captured paths record: the post-CFG combine, add_noise,
    scale_model_input and the 2B-row stacking between two queries are ONE launch (ctta_consistency_renoise) and the final
    combine is ctta_cfg_combine; a scale the kernels cannot reproduce bit for bit is combined by torch (`_cfg_rows`).
    `B`: rows of one CFG half."""

    def __init__(self, B, w_post, dev):
        self.B = self.rows = B
        self.w_post, self.dev = w_post, dev
        self.copies = 2 if w_post > 1. else 1
        self.w_dev = torch.full((B,), float(w_post), dtype=torch.float32, device=dev) if w_post > 1. else None

    def _w(self, unc):
        return N.ptr(self.w_dev) if unc is not None else N.c_void_p(0)

    def head(self, sch, t_head, first):
        """In the 18-step state.  Torch's own path, as the eager sampler starts: these launches are what bench.py times."""
        z_N = first * sch.init_noise_sigma
        return sch.scale_model_input(torch.cat([z_N] * 2) if self.copies == 2 else z_N, t_head)

    def start(self, sch, head, first, times, whole):
        return head

    def step(self, zh, draw, sig, z_in):
        cond, unc = _cfg_rows(zh, self.rows, self.w_post)
        N.check(N.lib().ctta_consistency_renoise(N.ptr(cond), N.ptr(unc), self._w(unc), N.ptr(draw), N.ptr(sig), N.ptr(z_in),
                                                 self.copies, self.B, zh[0].numel(), N.stream_ptr()))

    def end(self, zh):
        cond, unc = _cfg_rows(zh, self.rows, self.w_post)
        if unc is None:
            return cond
        out = torch.empty_like(unc)
        N.check(N.lib().ctta_cfg_combine(N.ptr(unc), N.ptr(cond), N.ptr(self.w_dev), N.ptr(out), self.B, zh[0].numel(),
                                         N.stream_ptr()))
        return out


class Keep(Plain):
    """`Plain` with a source clip, the sampler of `edit_latent`: after every query x0 becomes keep * src + (1 - keep) * x0
    inside the step's ONE launch (ctta_consistency_edit_renoise); the end is the combine and the blend in one launch
    (ctta_cfg_combine_keep), with or without post-CFG.  Inpainting starts from keep * src (x0 = 0 before the blend) noised
    at the head of the 18-step table, a variation from the whole source noised at the first remaining time."""

    def __init__(self, src_latent, keep_mask, w_post):
        if not src_latent.is_cuda:
            raise N.CttaError("src_latent is on %s: the HIP sampler has no CPU path" % src_latent.device)
        B, _, H, W = src_latent.shape
        super().__init__(B, w_post, src_latent.device)
        self.src = src_latent.detach().to(torch.float32).contiguous()
        self.keep = _keep_plane(keep_mask, B, H, W, self.dev)

    def head(self, sch, t_head, first):
        return sch._sigma_dev(sch.index_for_timestep(t_head), self.B, self.dev)

    def start(self, sch, head, first, times, whole):
        z_in = torch.empty((self.copies * self.B,) + tuple(self.src.shape[1:]), dtype=torch.float32, device=self.dev)
        if whole:
            self.step(None, first, head, z_in)
        else:
            sig = sch._sigma_dev(sch.index_for_timestep(times[0]), self.B, self.dev)
            N.check(N.lib().ctta_consistency_renoise(N.ptr(self.src), N.c_void_p(0), N.c_void_p(0), N.ptr(first), N.ptr(sig),
                                                     N.ptr(z_in), self.copies, self.B, self.src[0].numel(), N.stream_ptr()))
        return z_in

    def step(self, zh, draw, sig, z_in):
        cond, unc = _cfg_rows(zh, self.rows, self.w_post)
        N.check(N.lib().ctta_consistency_edit_renoise(N.ptr(cond), N.ptr(unc), self._w(unc), N.ptr(self.src), N.ptr(self.keep),
                                                      N.ptr(draw), N.ptr(sig), N.ptr(z_in), self.copies, self.B,
                                                      self.src[0].numel(), self.keep.shape[1], N.stream_ptr()))

    def end(self, zh):
        cond, unc = _cfg_rows(zh, self.rows, self.w_post)
        out = torch.empty_like(self.src)
        N.check(N.lib().ctta_cfg_combine_keep(N.ptr(unc), N.ptr(cond), self._w(unc), N.ptr(self.src), N.ptr(self.keep),
                                              N.ptr(out), self.B, self.src[0].numel(), self.keep.shape[1], N.stream_ptr()))
        return out


class Windows(Plain):
    """The sampler of `generate_long_latent` / `edit_long_latent`: a clip of `Ht` rows queried as n overlapping windows
    (rows b * n + k).  The post-CFG combine per window, the weighted overlap-add into one long x0, with a source the blend
    keep * src + (1 - keep) * x0, add_noise with ONE long draw, scale_model_input, the cut into the next windows and the
    2 x stacking are ONE launch (ctta_window_fuse_renoise; with a source ctta_window_fuse_edit_renoise), which is also the
    start (x0 = 0) and the end (no draw: the fused x0 goes to `x0_long`).  A variation starts with an all-ones keep plane.
    `plan`: `long_plan`'s (starts, weights).  `cache`: where the device weights, keyed (Ht, wh, n, overlap, device), and
    the all-ones plane, keyed (B, Ht * W, device), stay: they are uploaded once per layout and device, so a capture's
    warm-up run leaves them there and the recorded sequence holds no host -> device copy."""

    def __init__(self, plan, shape, overlap, w_post, dev, cache, src_latent=None, keep_mask=None):
        B, C, Ht, W = shape
        starts, weights = plan
        n, wh = weights.shape
        super().__init__(B, w_post, dev)
        self.rows, self.n, self.shape, self.wh, self.cache = B * n, n, tuple(shape), wh, cache
        self.src = self.keep = None
        if src_latent is not None:
            if not src_latent.is_cuda:
                raise N.CttaError("src_latent is on %s: the HIP sampler has no CPU path" % src_latent.device)
            self.src = src_latent.detach().to(torch.float32).contiguous()
            self.keep = _keep_plane(keep_mask, B, Ht, W, dev)
        self.starts = (N.c_int32 * n)(*starts)
        self.weights = _once(cache, (Ht, wh, n, int(overlap), str(dev)), lambda: weights.to(dev))

    head = Keep.head

    def _fuse(self, zh, keep, draw, sig, z_in, x0_long):
        B, C, Ht, W = self.shape
        cond, unc = _cfg_rows(zh, self.rows, self.w_post)
        outs = (N.ptr(cond), N.ptr(unc), self._w(unc), self.starts, N.ptr(self.weights))
        rest = (N.ptr(draw), N.ptr(sig), N.ptr(x0_long), N.ptr(z_in), self.copies, B, self.n, C, self.wh, Ht, W, N.stream_ptr())
        if self.src is None:
            N.check(N.lib().ctta_window_fuse_renoise(*outs, *rest))
        else:
            N.check(N.lib().ctta_window_fuse_edit_renoise(*outs, N.ptr(self.src), N.ptr(keep), *rest))

    def start(self, sch, head, first, times, whole):
        B, C, Ht, W = self.shape
        z_in = torch.empty((self.copies * self.rows, C, self.wh, W), dtype=torch.float32, device=self.dev)
        keep = self.keep
        if not whole:
            head = sch._sigma_dev(sch.index_for_timestep(times[0]), B, self.dev)
            keep = _once(self.cache, (B, Ht * W, str(self.dev)),
                         lambda: torch.ones(B, Ht * W, dtype=torch.float32, device=self.dev))
        self._fuse(None, keep, first, head, z_in, None)
        return z_in

    def step(self, zh, draw, sig, z_in):
        self._fuse(zh, self.keep, draw, sig, z_in, None)

    def end(self, zh):
        out = torch.empty(self.shape, dtype=torch.float32, device=self.dev)
        self._fuse(zh, self.keep, None, None, None, out)
        return out


def sample(form, unet, sch, states, mask, draw, num_steps, cfg_scale_input, r=None, reuse_text=True, **unet_kw):
    """The few-step sampler on a step form: the last `r` (None: all) of the `num_steps` query times run, one launch of the
    form between two queries.  `states` / `mask`: the stacked text states (`stack_text`).  `draw(k)`: the k-th noise, read
    when its step comes.  `reuse_text`: queries after the first take the text K / V from the handle's cache on the caller's
    word (the text states are the same tensors for the whole call, the teacher loop's rule); False leaves the decision to
    the module on every query.  Nothing but launches happens once `draw(k)` is a tensor at hand."""
    first = sch._check(draw(0))
    times, head = query_times(sch, num_steps, first.device, r, lambda t_head: form.head(sch, t_head, first))
    z_in = form.start(sch, head, first, times, len(times) == int(num_steps))
    for k, t in enumerate(times):
        zh = unet(z_in, t, guidance=cfg_scale_input, encoder_hidden_states=states, encoder_attention_mask=mask,
                  reuse_text=(k > 0) if reuse_text else None, **unet_kw).sample
        if k == len(times) - 1:
            break
        sig = sch._sigma_dev(sch.index_for_timestep(times[k + 1]), form.B, first.device)
        z_in = torch.empty_like(zh)
        form.step(zh, sch._check(draw(k + 1)), sig, z_in)
    return form.end(zh)
