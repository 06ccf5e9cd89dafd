"""CPU-only checks of the host plumbing in consistencytta_amd/models.py that the GPU suite reaches only as a side effect:
the autograd bridge to the engine's backward, the train / eval mode table of both distillation models, the hardware-queue
placement search (fake streams, fake clock) and the path choice of `do_ema_update` (fake library)."""
import contextlib

import pytest
import torch
from torch import nn

import cases
from consistencytta_amd import _native as N
from consistencytta_amd import models


# ------------------------------------------------------------------------------------------------
class _RecordingModel:
    def __init__(self):
        self.calls = []

    def _student_backward(self, *args):
        self.calls.append(args)


@pytest.mark.parametrize("n_saved", [4, 3])      # AudioLCM saves pred, target, sigma, gamma; AudioGDM pred, target, weights
def test_engine_loss_hands_saved_values_and_the_gradient_to_student_backward(n_saved):
    saved = tuple(object() for _ in range(n_saved))
    for factor in (1.0, 2.0):
        model = _RecordingModel()
        anchor = torch.zeros((), requires_grad=True)
        loss = torch.tensor(0.75)
        out = models._EngineLoss.apply(anchor, loss, model, *saved)
        assert out is not loss and out.data_ptr() != loss.data_ptr()      # a clone, not the input tensor
        assert float(out.detach()) == 0.75 and out.requires_grad
        assert model.calls == []
        (out if factor == 1.0 else factor * out).backward()
        assert len(model.calls) == 1
        args = model.calls[0]
        assert len(args) == n_saved + 1
        assert all(a is s for a, s in zip(args, saved))                   # the saved values, in order
        assert type(args[-1]) is float and args[-1] == factor             # the incoming gradient as a Python float
        assert anchor.grad is None                                        # one None per input: nothing flows back


# ------------------------------------------------------------------------------------------------
_KW = dict(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
           unet_model_config_path="tiny_light.json", unet_config=cases.TINY_UNET, snr_gamma=5.0, teacher_guidance_scale=-1)


def _lcm():
    return models.AudioLCM(use_edm=True, num_diffusion_steps=18, vae=nn.Linear(2, 2), loss_type="mse",
                           text_encoder=nn.Linear(2, 2), tokenizer=object(), **_KW)


def _gdm():
    return models.AudioGDM(text_encoder=nn.Linear(2, 2), tokenizer=object(), **_KW)


@pytest.mark.parametrize("make", [_lcm, _gdm])
def test_train_keeps_every_frozen_module_in_eval_mode(make):
    m = make()
    frozen = [m.teacher_unet, m.student_ema_unet, m.text_encoder]
    if isinstance(m, models.AudioLCM):
        frozen += [m.student_target_unet, m.vae]
    for f in frozen:
        f.train()
    assert m.train() is m
    assert m.training and m.student_unet.training
    assert all(not f.training for f in frozen)
    m.check_eval_mode()
    assert m.eval() is m
    assert not m.training and not m.student_unet.training
    assert all(not f.training for f in frozen)
    with pytest.raises(AssertionError, match="EMA update should only be called during training"):
        m.update_ema()
    with pytest.raises(AssertionError, match="EMA update should only be called during training"):
        m._optimizer_tail(None, None, 1.0, True)
    m.teacher_unet.train()
    with pytest.raises(AssertionError, match="The teacher_unet is not in eval mode."):
        m.check_eval_mode()
    if isinstance(m, models.AudioLCM):
        m.train()
        m.student_target_unet.train()
        with pytest.raises(AssertionError, match="The student_target_unet is not in eval mode."):
            m.check_eval_mode()


# ------------------------------------------------------------------------------------------------
class _FakeStream:
    def __init__(self, name):
        self.name = name

    def wait_stream(self, other):
        pass


class _FakeCuda:
    """torch.cuda's timing surface on a clock that only `run_on` advances."""

    def __init__(self, monkeypatch):
        self.now = 0.0
        self.cur = _FakeStream("cur")
        fake = self

        class Event:
            def __init__(self, enable_timing=False):
                assert enable_timing
                self.t = None

            def record(self, stream=None):
                assert stream is None or stream is fake.cur
                self.t = fake.now

            def elapsed_time(self, other):
                return other.t - self.t

        monkeypatch.setattr(torch.cuda, "Event", Event)
        monkeypatch.setattr(torch.cuda, "synchronize", lambda dev=None: None)
        monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: fake.cur)


def _search(monkeypatch, costs):
    """Runs the placement search over len(costs) fake streams; costs[i] = (ms of pass 1, ms of pass 2) on stream i.
    Returns (index of the chosen stream, the tried list, the streams `run_on` saw in order)."""
    cuda = _FakeCuda(monkeypatch)
    cands = [_FakeStream(i) for i in range(len(costs))]
    seen = []

    def run_on(s):
        cuda.now += costs[s.name][sum(1 for x in seen if x is s)]
        seen.append(s)
    best, tried = models._place_stream(cands, run_on, "cuda:0")
    return cands.index(best), tried, [s.name for s in seen]


def test_placement_search_selection_rules(monkeypatch):
    """The rules of `_DistillStepGraph._place_teacher_stream` as it stood before the search became one function
    (consistencytta_amd/models.py:1540-1557 at commit 10dade0): `for _ in range(2)` with `ms` overwritten, so the SECOND
    pass counts (:1542-1553); `self.placement_ms.append(round(ms, 2))`, one entry per candidate (:1554);
    `if ms < best[1]`, strict, so the first candidate wins a tie (:1555-1556); the winner becomes the stream (:1557).
    `capture_pipeline` spelled the same loop (:2014-2036)."""
    # the minimum of the second passes wins, whatever the first passes cost
    best, tried, seen = _search(monkeypatch, [(1.0, 9.0), (50.0, 3.0), (2.0, 5.0)])
    assert best == 1 and tried == [9.0, 3.0, 5.0]
    assert seen == [0, 0, 1, 1, 2, 2]                 # every candidate exactly twice, in order
    # ties: the first candidate stays (the comparison is on the unrounded time)
    best, tried, _ = _search(monkeypatch, [(7.0, 4.0), (7.0, 4.0), (7.0, 6.0), (7.0, 4.0)])
    assert best == 0 and tried == [4.0, 4.0, 6.0, 4.0]
    best, tried, _ = _search(monkeypatch, [(0.0, 4.004), (0.0, 4.001), (0.0, 9.0)])
    assert best == 1 and tried == [4.0, 4.0, 9.0]          # rounded to 2 decimals in the list only
    best, tried, _ = _search(monkeypatch, [(0.0, 1.23456), (0.0, 2.0), (0.0, 3.0)])
    assert best == 0 and tried == [1.23, 2.0, 3.0]


# ------------------------------------------------------------------------------------------------
class _FakeLib:
    def __init__(self):
        self.launches = []

    def ctta_ema_update2(self, src, a, decay_a, b, decay_b, n, stream):
        self.launches.append((src.value, a.value, decay_a, b.value, decay_b, n))
        return 0


class _FakeFlat:
    device = "cuda:0"

    def __init__(self, addr, n=64):
        self.addr, self.n = addr, n

    def numel(self):
        return self.n

    def data_ptr(self):
        return self.addr


class _FakeParam:
    """A parameter that claims to live on the device; `detach()` gives a real tensor so that version bumps show."""

    def __init__(self, n, is_cuda=True):
        self.t = torch.zeros(n)
        self.is_cuda = is_cuda

    def detach(self):
        return self.t.detach()

    def numel(self):
        return self.t.numel()


class _FakeNet:
    def __init__(self, flat=None, is_cuda=True):
        self._flat = flat
        self._rehome_count = 0
        self.current = True
        self.marked = 0
        self.params = {"a.weight": _FakeParam(6, is_cuda), "b.bias": _FakeParam(2, is_cuda)}

    def named_parameters(self):
        return self.params.items()

    def flat_is_current(self):
        return self.current

    def mark_weights_changed(self):
        self.marked += 1


@pytest.fixture
def fake_lib(monkeypatch):
    L = _FakeLib()
    monkeypatch.setattr(N, "lib", lambda: L)
    monkeypatch.setattr(N, "stream_ptr", lambda: N.c_void_p(0))
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    return L


def test_do_ema_update_first_call_validates_then_the_steady_state_is_one_launch(fake_lib):
    src, tgt, ema = (_FakeNet(_FakeFlat(0x1000 * (i + 1))) for i in range(3))
    assert getattr(src, "_ema_validated", None) is None
    models.do_ema_update(src, [tgt, ema], [0.95, 0.999])
    sig = tuple((id(m), 0) for m in (src, tgt, ema))
    assert fake_lib.launches == [(0x1000, 0x2000, 0.95, 0x3000, 0.999, 64)]
    assert src._ema_validated == sig and (tgt.marked, ema.marked) == (1, 1)
    # steady state: one launch over the flats, without looking at the parameters again
    src.named_parameters = tgt.named_parameters = ema.named_parameters = None
    models.do_ema_update(src, [tgt, ema], [0.95, 0.999])
    assert fake_lib.launches[1:] == [(0x1000, 0x2000, 0.95, 0x3000, 0.999, 64)]
    assert (tgt.marked, ema.marked) == (2, 2) and src._ema_validated == sig
    # one shadow: the second slot is NULL with decay 0
    src1, ema1 = _FakeNet(_FakeFlat(0x5000)), _FakeNet(_FakeFlat(0x6000))
    models.do_ema_update(src1, [ema1], [0.999])
    assert fake_lib.launches[2:] == [(0x5000, 0x6000, 0.999, None, 0.0, 64)]
    assert src1._ema_validated == ((id(src1), 0), (id(ema1), 0))
    with pytest.raises(AssertionError):
        models.do_ema_update(src1, [ema1], [1.5])


def test_do_ema_update_without_flats_launches_per_parameter_and_bumps_versions(fake_lib):
    src, tgt, ema = _FakeNet(), _FakeNet(), _FakeNet()
    versions = [p.t._version for net in (tgt, ema) for p in net.params.values()]
    models.do_ema_update(src, [tgt, ema], [0.95, 0.999])
    assert [(l[2], l[4], l[5]) for l in fake_lib.launches] == [(0.95, 0.999, 6), (0.95, 0.999, 2)]
    for l, name in zip(fake_lib.launches, src.params):
        assert l[0] == src.params[name].t.data_ptr() and l[1] == tgt.params[name].t.data_ptr()
        assert l[3] == ema.params[name].t.data_ptr()
    assert [p.t._version for net in (tgt, ema) for p in net.params.values()] == [v + 1 for v in versions]
    assert getattr(src, "_ema_validated", None) is None and (tgt.marked, ema.marked) == (0, 0)
    # a flat buffer that is no longer current takes the same path
    a, b = _FakeNet(_FakeFlat(0x1000)), _FakeNet(_FakeFlat(0x2000))
    b.current = False
    del fake_lib.launches[:]
    models.do_ema_update(a, [b], [0.9])
    assert len(fake_lib.launches) == 2 and getattr(a, "_ema_validated", None) is None


def test_do_ema_update_refuses_cpu_parameters(fake_lib):
    src, ema = _FakeNet(is_cuda=False), _FakeNet(is_cuda=False)
    with pytest.raises(N.CttaError, match=r"EMA update needs CUDA\(ROCm\) parameters; there is no CPU path"):
        models.do_ema_update(src, [ema], [0.999])
    assert fake_lib.launches == []
