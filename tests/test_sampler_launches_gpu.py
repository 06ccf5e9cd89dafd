"""The launch sequence of every form of the few-step sampler (consistencytta_amd/sampler.py: plain, keep, windows, windows
with a source), pinned call by call: which sampler entry runs at the start, between two U-Net queries and at the end, with
which NULL pointers and counts, and what every query is told about the text K / V.  The expected lists are written out from
the sequences the four separate loops issued before they were folded into one; nothing here is recorded from the code under
test.  The values the launches compute are pinned elsewhere (test_serving_gpu, test_edit_gpu, test_long_gpu,
test_long_edit_gpu); this file keeps a launch from being added, dropped or reordered inside a captured graph."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from consistencytta_amd import _native as N  # noqa: E402
from test_long_edit_gpu import _kw, _pipe, _source, _states, _time_mask  # noqa: E402

DEV = "cuda:0"
B, C, H, W = 2, 8, 32, 16
HT, WINDOW_H = 48, 32
# overlap -> windows of long_plan(48, 32, overlap): ceil((48 - 32) / (32 - overlap)) + 1
LAYOUTS = {24: 3, 16: 2}
W_IN = 4.0
POSTS = (1.0, 2.0, 1.3)
# whether the step kernels take the uncond rows and combine themselves: 1 - 2.0 is exact in fp32, 1 - 1.3 is not (torch
# combines first, the kernel sees cond rows only), 1.0 is no post-CFG
KERNEL_COMBINES = {1.0: False, 2.0: True, 1.3: False}
SAMPLER_ENTRIES = ("ctta_heun_", "ctta_consistency_", "ctta_cfg_combine", "ctta_window_fuse_")

# entry -> the scalar arguments logged, by position in include/ctta.h; pointers are logged as labels (`_Recorder.label`)
POINTERS = {
    "ctta_consistency_renoise": dict(cond=0, uncond=1),
    "ctta_consistency_edit_renoise": dict(cond=0, uncond=1),
    "ctta_cfg_combine_keep": dict(uncond=0),
    "ctta_window_fuse_renoise": dict(cond=0, uncond=1, noise=5, x0_long=7, out=8),
    "ctta_window_fuse_edit_renoise": dict(cond=0, uncond=1, keep=6, noise=7, x0_long=9, out=10),
}
INTS = {
    "ctta_consistency_renoise": dict(copies=6),
    "ctta_consistency_edit_renoise": dict(copies=8),
    "ctta_window_fuse_renoise": dict(copies=9, batch=10, n_windows=11),
    "ctta_window_fuse_edit_renoise": dict(copies=11, batch=12, n_windows=13),
}


class _Recorder:
    """Stands in front of the library: logs the sampler's entries, calls the real entry, passes everything else through."""

    def __init__(self, real, named):
        self._real, self._named, self.log = real, named, []

    def label(self, p):
        """NULL -> None, a tensor the test handed in -> its name, anything else -> "set"."""
        v = getattr(p, "value", p)
        return None if not v else self._named.get(v, "set")

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith(SAMPLER_ENTRIES):
            return fn

        def logged(*a):
            rec = {k: self.label(a[i]) for k, i in POINTERS.get(name, {}).items()}
            rec.update({k: int(a[i]) for k, i in INTS.get(name, {}).items()})
            self.log.append((name[len("ctta_"):], rec))
            return fn(*a)
        return logged


@pytest.fixture(scope="module")
def shared():
    pipe, cfg = _pipe()
    enc, mask = _states(cfg, "launches")
    return pipe, cfg, enc, mask


def _record(monkeypatch, pipe, call, **named):
    """The filtered log of `call()`: sampler entries and `("Q", reuse_text)` per U-Net query, in issue order."""
    rec = _Recorder(N.lib(), {t.data_ptr(): k for k, t in named.items()})
    forward = pipe.unet.forward

    def query(*a, **kw):
        rec.log.append(("Q", kw.get("reuse_text")))
        return forward(*a, **kw)
    monkeypatch.setattr(N, "lib", lambda: rec)
    monkeypatch.setattr(pipe.unet, "forward", query)
    call()
    torch.cuda.synchronize()
    monkeypatch.undo()
    return rec.log


def _noise(steps, h, seed):
    return torch.randn((steps, B, C, h, W), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _uncond(post):
    return "set" if KERNEL_COMBINES[post] else None


def _copies(post):
    return 2 if post > 1 else 1


@pytest.mark.parametrize("post", POSTS)
def test_plain_form(shared, monkeypatch, post):
    pipe, cfg, enc, mask = shared
    steps = 3
    kw = _kw(cfg, post, "launches")
    noise = _noise(steps, H, 1)
    log = _record(monkeypatch, pipe, lambda: pipe._generate_latent_static(
        enc, mask, noise, W_IN, post, steps, kw.get("uncond_states"), kw.get("uncond_mask")))
    want = [("heun_scale_model_input", {}), ("Q", False)]
    want += [("consistency_renoise", dict(cond="set", uncond=_uncond(post), copies=_copies(post))), ("Q", True)] * (steps - 1)
    if KERNEL_COMBINES[post]:           # torch combines 1.3 itself; without post-CFG nothing ends the loop
        want.append(("cfg_combine", {}))
    assert log == want


@pytest.mark.parametrize("post", POSTS)
@pytest.mark.parametrize("strength,steps", [(1.0, 3), (0.5, 4)])
def test_keep_form(shared, monkeypatch, post, strength, steps):
    pipe, cfg, enc, mask = shared
    r = steps if strength == 1.0 else 2
    src, keep, noise = _source(H, 2), _time_mask(H, 8, 24), _noise(r, H, 3)
    log = _record(monkeypatch, pipe, lambda: pipe.edit_latent(
        enc, mask, noise[0], src, keep, strength, W_IN, post, steps, step_noise=noise[1:], **_kw(cfg, post, "launches")),
        src=src)
    step = ("consistency_edit_renoise", dict(cond="set", uncond=_uncond(post), copies=_copies(post)))
    if strength == 1.0:                 # inpainting: x0 = 0 before the blend
        want = [("consistency_edit_renoise", dict(cond=None, uncond=None, copies=_copies(post)))]
    else:                               # variation: the whole source, noised
        want = [("consistency_renoise", dict(cond="src", uncond=None, copies=_copies(post)))]
    want += [("Q", None)] + [step, ("Q", None)] * (r - 1)       # the eager entry leaves the text K / V to the module
    want.append(("cfg_combine_keep", dict(uncond=_uncond(post))))
    assert log == want


def _window_launch(post, n, cond="set", noise="set", out="set", x0_long=None, **more):
    uncond = _uncond(post) if cond else None
    return dict(cond=cond, uncond=uncond, noise=noise, x0_long=x0_long, out=out, copies=_copies(post), batch=B, n_windows=n,
                **more)


@pytest.mark.parametrize("post", POSTS)
@pytest.mark.parametrize("overlap", sorted(LAYOUTS))
def test_windows_form(shared, monkeypatch, post, overlap):
    pipe, cfg, enc, mask = shared
    steps, n = 3, LAYOUTS[overlap]
    noise = _noise(steps, HT, 4)
    log = _record(monkeypatch, pipe, lambda: pipe.generate_long_latent(
        enc, mask, noise[0], W_IN, post, steps, overlap, WINDOW_H, step_noise=noise[1:], **_kw(cfg, post, "launches")))
    name = "window_fuse_renoise"
    want = [(name, _window_launch(post, n, cond=None)), ("Q", False)]
    want += [(name, _window_launch(post, n)), ("Q", True)] * (steps - 1)
    want.append((name, _window_launch(post, n, noise=None, out=None, x0_long="set")))
    assert log == want


@pytest.mark.parametrize("post", POSTS)
@pytest.mark.parametrize("overlap", sorted(LAYOUTS))
@pytest.mark.parametrize("strength,steps", [(1.0, 3), (0.5, 4)])
def test_windows_form_with_a_source(shared, monkeypatch, post, overlap, strength, steps):
    pipe, cfg, enc, mask = shared
    n = LAYOUTS[overlap]
    r = steps if strength == 1.0 else 2
    src, keep, noise = _source(HT, 5), _time_mask(HT, 16, 40), _noise(r, HT, 6)
    log = _record(monkeypatch, pipe, lambda: pipe.edit_long_latent(
        enc, mask, noise[0], src, keep, strength, W_IN, post, steps, overlap, WINDOW_H, step_noise=noise[1:],
        **_kw(cfg, post, "launches")), mask=keep)
    name = "window_fuse_edit_renoise"
    # a variation starts from the whole source: the all-ones plane stands where the mask does
    want = [(name, _window_launch(post, n, cond=None, keep="mask" if strength == 1.0 else "set")), ("Q", False)]
    want += [(name, _window_launch(post, n, keep="mask")), ("Q", True)] * (r - 1)
    want.append((name, _window_launch(post, n, noise=None, out=None, x0_long="set", keep="mask")))
    assert log == want
