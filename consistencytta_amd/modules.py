"""Drop-in nn.Module mirrors of the reference's numerical modules, backed by libctta_hip.so.

Same constructor configs, `forward` signatures, `state_dict` key names / order and error
behaviour as
  * diffusers.UNet2DConditionGuidedModel  (diffusers/models/unet_2d_condition_guided.py:51)
  * diffusers.UNet2DConditionModel        (diffusers/models/unet_2d_condition.py)  [teacher]
  * audioldm AutoencoderKL                (audioldm/variational_autoencoder/autoencoder.py:10)
  * audioldm.hifigan.Generator            (audioldm/hifigan/models.py:72)
so the reference's L4 callers (`models/audio_consistency_model.py`, `inference.py`,
`easy_inference/consistencytta.py`) can switch by changing an import.  The modules only OWN
parameters (fp32, reference layout); all arithmetic happens in the HIP engines, which keep
their own packed bf16 copies and are re-synced when parameter versions change.
"""
import json
import math
from collections import OrderedDict
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

from . import _native as N
from . import spec


@dataclass
class UNet2DConditionOutput:
    sample: torch.Tensor


class _ParamTree(nn.Module):
    """Registers parameters under dotted reference key names (nested anonymous modules)."""

    def _register(self, table, frozen=()):
        self._frozen_keys = tuple(frozen)
        for key, shape in table.items():
            mod = self
            parts = key.split(".")
            for p in parts[:-1]:
                if p not in mod._modules:
                    mod.add_module(p, nn.Module())
                mod = mod._modules[p]
            param = nn.Parameter(torch.empty(*shape, dtype=torch.float32), requires_grad=key not in frozen)
            mod.register_parameter(parts[-1], param)

    def init_deterministic(self, seed=0, prefix=""):
        """Random init from the build's deterministic generator (spec.det_weight)."""
        with torch.no_grad():
            for k, p in self.named_parameters():
                p.copy_(torch.from_numpy(spec.det_weight(prefix + k, tuple(p.shape), seed)).to(p.device))
        return self

    def init_random_(self, seed=0, prefix=""):
        """Fast on-device random init with the same scale rule (benchmarks: values need not be
        reproducible across boxes, only well-conditioned)."""
        gen = torch.Generator(device=self.device if hasattr(self, "device") else "cpu")
        gen.manual_seed(seed)
        with torch.no_grad():
            for k, p in self.named_parameters():
                off, amp = spec.weight_rule(prefix + k, tuple(p.shape))
                p.copy_(off + amp * (torch.rand(p.shape, generator=gen, device=p.device) * 2 - 1))
        return self

    def _weights_version(self):
        return sum(self._weights_versions())

    def _weights_versions(self):
        """(base part, adapter part): the adapter part covers the parameters whose key names a LoRA tensor (`_lora.`), so
        a handle can tell "only the adapters moved" (re-pack them alone) from a change of the base."""
        base = 7 * getattr(self, "_manual_version", 0)
        adapters = 7 * getattr(self, "_manual_adapter_version", 0)
        for k, p in self.named_parameters():
            v = p._version + 1000003 * (p.data_ptr() % 1000003)
            if "_lora." in k:
                adapters += v
            else:
                base += v
        return base, adapters

    def mark_weights_changed(self, adapters_only=False):
        """Call after parameters were updated through raw pointers (fused AdamW / EMA kernels).  `adapters_only`: the
        pass walked the LoRA adapters alone (the trainable prefix of a module with `lora_rank`)."""
        if adapters_only:
            self._manual_adapter_version = getattr(self, "_manual_adapter_version", 0) + 1
        else:
            self._manual_version = getattr(self, "_manual_version", 0) + 1

    def flatten_parameters_(self):
        """Re-homes every parameter into ONE contiguous fp32 buffer (views keep names/shapes), so the
        optimizer, EMA and gradient all-reduce run as single launches over the whole model.
        Returns the flat buffer; `flat_grad_()` gives the matching gradient buffer."""
        params = self._flat_order()
        flat0 = getattr(self, "_flat", None)
        if flat0 is not None and all(
                flat0.data_ptr() <= p.data_ptr() < flat0.data_ptr() + flat0.numel() * 4 for p in params):
            return flat0
        total = sum(p.numel() for p in params)
        flat = torch.empty(total, dtype=torch.float32, device=params[0].device)
        off = 0
        for p in params:
            n = p.numel()
            flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = flat[off:off + n].view(p.shape)
            off += n
        self._flat = flat
        self._flat_grad = None
        self._flat_checked_at = getattr(self, "_rehome_count", 0)
        return flat

    # Everything that re-homes `p.data` through the nn.Module protocol (.to() / .float() / .cuda() / ... and
    # load_state_dict(assign=True)) bumps a counter, so `flat_is_current()` is O(1) on the steady-state training step
    # instead of a walk over 690 parameters per network (0.9 ms of host time per EMA update in round 2's bench).
    def _apply(self, fn, recurse=True):
        self._rehome_count = getattr(self, "_rehome_count", 0) + 1
        return super()._apply(fn, recurse)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        if assign:
            self._rehome_count = getattr(self, "_rehome_count", 0) + 1
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    def flat_is_current(self):
        """True while every parameter still aliases `_flat` (a later `.to()`, `.float()`, `load_state_dict(assign=True)`
        ... re-homes `p.data` and would leave the fused optimizer / EMA kernels updating a stale buffer).  The walk over
        the parameters runs once per re-homing event (see `_apply`); assigning `p.data` by hand is not tracked."""
        flat = getattr(self, "_flat", None)
        if flat is None:
            return False
        epoch = getattr(self, "_rehome_count", 0)
        if getattr(self, "_flat_checked_at", None) == epoch:
            return True
        lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
        ok = all(lo <= p.data_ptr() < hi for p in self.parameters())
        if ok:
            self._flat_checked_at = epoch
        return ok

    def grads_alias_flat(self):
        """True while every trainable parameter's `.grad` is a view of `_flat_grad` (`zero_grad(set_to_none=True)`
        followed by a backward that allocates fresh gradients would break this)."""
        g = getattr(self, "_flat_grad", None)
        if g is None:
            return False
        lo, hi = g.data_ptr(), g.data_ptr() + g.numel() * 4
        return all(p.grad is not None and lo <= p.grad.data_ptr() < hi for p in self.parameters() if p.requires_grad)

    def grads_alias_flat_sampled(self, k=8):
        """The per-step form of `grads_alias_flat` (called by FusedAdamW.step): the first and the last trainable parameter
        plus `k` more, rotating from call to call.  What breaks the aliasing in practice -- `zero_grad(set_to_none=True)`
        followed by a backward that allocates fresh gradients -- breaks it for EVERY parameter and is seen by the very
        next call; a single hand-assigned `p.grad` is seen within n / k calls.  The full walk costs 690 `p.grad` look-ups =
        1.5-3 ms of host time per optimizer step, more than the AdamW kernel itself on a slow host (round 4: 3.48 vs
        2.78 ms for the same launch on two boxes -- it was this walk inside the timed bracket)."""
        g = getattr(self, "_flat_grad", None)
        if g is None:
            return False
        tr = getattr(self, "_trainable_cache", None)
        key = (getattr(self, "_rehome_count", 0), tuple(getattr(self, "_frozen_keys", ())))
        if tr is None or tr[0] != key:
            tr = self._trainable_cache = (key, [p for p in self.parameters() if p.requires_grad])
            self._alias_cursor = 0
            self._alias_calls = 0
            return self.grads_alias_flat()
        ps = tr[1]
        n = len(ps)
        if n == 0:
            return True
        # every 64th call walks everything (a single hand-assigned p.grad is then seen within 64 steps whatever n / k is)
        self._alias_calls = getattr(self, "_alias_calls", 0) + 1
        if self._alias_calls % 64 == 0:
            return self.grads_alias_flat()
        lo, hi = g.data_ptr(), g.data_ptr() + g.numel() * 4
        cur = self._alias_cursor
        idx = [0, n - 1] + [(cur + i) % n for i in range(k)]
        self._alias_cursor = (cur + k) % n
        for i in idx:
            p = ps[i]
            if not p.requires_grad:       # frozen after the cache was built (requires_grad_(False) by hand): rebuild, walk
                self._trainable_cache = None
                return self.grads_alias_flat()
            gr = p.grad
            if gr is None or not (lo <= gr.data_ptr() < hi):
                # the sample says no: let the full walk decide (it filters on requires_grad at call time) before step() raises
                return self.grads_alias_flat()
        return True

    def realias_grads_(self):
        """Points every trainable `p.grad` back at its slice of the flat gradient buffer (after set_to_none)."""
        g = getattr(self, "_flat_grad", None)
        if g is None:
            return
        off = 0
        for p in self._flat_order():
            n = p.numel()
            if p.requires_grad and (p.grad is None or p.grad.data_ptr() != g.data_ptr() + off * 4):
                p.grad = g[off:off + n].view(p.shape)
            off += n

    def flat_grad_(self):
        """Flat fp32 gradient buffer aliased by every `p.grad` (zero-initialised on first use)."""
        flat = self.flatten_parameters_()
        if getattr(self, "_flat_grad", None) is None:
            g = torch.zeros_like(flat)
            off = 0
            for p in self._flat_order():
                n = p.numel()
                if p.requires_grad:
                    p.grad = g[off:off + n].view(p.shape)
                off += n
            self._flat_grad = g
        return self._flat_grad

    def _flat_order(self):
        """Trainable parameters first (state-dict order), frozen ones last, so optimizer / all-reduce
        kernels cover exactly the prefix `[0, n_trainable())` of the flat buffers."""
        frozen = set(getattr(self, "_frozen_keys", ()))
        named = list(self.named_parameters())
        return [p for k, p in named if k not in frozen] + [p for k, p in named if k in frozen]

    def n_trainable(self):
        frozen = set(getattr(self, "_frozen_keys", ()))
        return sum(p.numel() for k, p in self.named_parameters() if k not in frozen)

    def _table(self, prefix_filter=None, strip=""):
        sd = OrderedDict()
        for k, p in self.named_parameters():
            if prefix_filter and not k.startswith(prefix_filter):
                continue
            if not p.is_cuda:
                raise N.CttaError(
                    "parameter '%s' is on %s: the HIP engine needs CUDA(ROCm) tensors; there is no CPU path"
                    % (k, p.device))
            sd[k[len(strip):] if strip and k.startswith(strip) else k] = p.detach()
        return sd

    # handles are not copyable / picklable: a deepcopy (audio_consistency_model.py:65) gets fresh ones
    @staticmethod
    def _without_handles(k, v):
        """(handled, value a copy gets): empty holders of the same kind, nothing native"""
        if isinstance(v, N.EngineHandle):
            return True, N.EngineHandle(v.destroy)
        if k == "_eng":
            return True, {w: [N.EngineHandle(e.destroy) for e in es] for w, es in v.items()}
        if k.startswith("_h_") or k in ("_vae_pending", "_voc_pending", "_anchor"):
            return True, None
        return False, v

    def __getstate__(self):
        return {k: self._without_handles(k, v)[1] for k, v in self.__dict__.items()}

    def __deepcopy__(self, memo):
        import copy
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            handled, fresh = self._without_handles(k, v)
            new.__dict__[k] = fresh if handled else None if k.startswith("_flat") else copy.deepcopy(v, memo)
        return new


def _cfg_get(cfg, key, default=None):
    return cfg[key] if key in cfg else default


class _UNetBase(_ParamTree):
    _guided = True

    def __init__(self, **config):
        super().__init__()
        cfg = dict(spec.LIGHT_UNET_CONFIG)
        cfg.update({k: v for k, v in config.items() if not k.startswith("_")})
        for k in ("down_block_types", "up_block_types"):
            for t in cfg[k]:
                if t not in ("CrossAttnDownBlock2D", "DownBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"):
                    raise ValueError(f"{t} does not exist.")  # unet_2d_blocks.py get_down_block
        if len(cfg["down_block_types"]) != len(cfg["up_block_types"]):
            raise ValueError("Must provide the same number of `down_block_types` as `up_block_types`.")
        if len(cfg["block_out_channels"]) != len(cfg["down_block_types"]):
            raise ValueError("Must provide the same number of `block_out_channels` as `down_block_types`.")
        if not cfg.get("use_linear_projection", True):
            raise ValueError("use_linear_projection=False (conv proj_in/out) is not supported by the HIP engine")
        self.config = SimpleNamespace(**cfg)
        self._cfg = cfg
        frozen = ("guidance_proj.weight",)  # embeddings.py:229 requires_grad=False
        self._register(spec.unet_param_spec(cfg, self._guided), frozen)
        self._engine = N.EngineHandle("ctta_unet_destroy")
        self.debug_taps = False
        self.enable_training = False   # True: the native handle also carries the backward pass
        self.lora_rank = 0             # > 0: adapters at the attention projections (enable_lora_)
        self.lora_scale = 1.0          # y = W x + lora_scale * up(down(x)); pushed to the handle before each call
        # the fused site kernels where they take the shapes: True (= 1) in the backward groups, 3 in the forward groups too
        # (measured slower than the launches they replace there, profiles/lora_step.txt), False: per-site launches everywhere
        self.lora_fused = True
        # per-request adapters (add_adapter): name -> slot of the handle's bank, slot -> (version, host-side tensors or
        # None for a slot to be zeroed), what the current handle holds, and the row table bound to it
        self.adapter_slots = 8         # slots of the bank a new handle gets; grows (to at most 64) with add_adapter
        self._adapters = OrderedDict()
        self._slot_state = {}
        self._adapter_ver = 0
        self._h_bank = None
        self._bank_loaded = {}
        self._h_rows = self._rows_key = self._rows_dev = None

    # ---- LoRA (audio_distilled_model.py:116-145 -> diffusers LoRAAttnProcessor, attention_processor.py:508-613)
    def enable_lora_(self, rank=4, generator=None):
        """Gives every attention projection (to_q / to_k / to_v / to_out of attn1 and attn2) a rank-`rank` adapter,
        y = W x + up(down(x)), and freezes every base parameter: what `setup_lora` does to the reference's student.
        The adapters are registered under the reference's key names (`...attn1.processor.to_q_lora.down.weight`), so the
        state dict has the reference's keys in its order; init as LoRALinearLayer: down ~ N(0, 1 / rank^2), up = 0.
        They are the only trainable parameters and therefore the prefix `[0, n_trainable())` of the flat parameter /
        gradient buffers (`_flat_order`), which is all the fused optimizer and EMA passes walk.  In place; returns self."""
        rank = int(rank)
        if self.lora_rank:
            if rank != self.lora_rank:
                raise ValueError("adapters of rank %d are already set up (asked for rank %d)" % (self.lora_rank, rank))
            return self
        if not 1 <= rank <= 16:
            raise ValueError("LoRA rank %d is outside what the HIP kernels take (1..16)" % rank)
        dev = self.device
        base = [k for k, _ in self.named_parameters()]
        for p in self.parameters():
            p.requires_grad_(False)
            p.grad = None
        for key, shape in spec.lora_param_spec(self._cfg, rank, self._guided).items():
            mod = self
            parts = key.split(".")
            for q in parts[:-1]:
                if q not in mod._modules:
                    mod.add_module(q, nn.Module())
                mod = mod._modules[q]
            if parts[-2] == "down":
                w = (torch.randn(*shape, generator=generator, dtype=torch.float32) / rank).to(dev)
            else:
                w = torch.zeros(*shape, dtype=torch.float32, device=dev)
            mod.register_parameter(parts[-1], nn.Parameter(w, requires_grad=True))
        self._frozen_keys = tuple(base)
        self.lora_rank = rank
        self._drop_flat_()
        return self

    def _drop_flat_(self):
        """The parameter set changed: the flat buffers, their caches and the packed copy in the handle are stale."""
        self._flat = self._flat_grad = self._trainable_cache = None
        self._rehome_count = getattr(self, "_rehome_count", 0) + 1
        self.mark_weights_changed()

    def lora_keys(self):
        return [k for k, _ in self.named_parameters() if "_lora." in k]

    # ---- per-request adapters: a bank of named adapter sets beside the module's own, one batch row -> one of them
    ADAPTER_SLOTS_MAX = 64

    def add_adapter(self, name, state_dict):
        """Registers the adapter set `state_dict` (the keys of `lora_keys()`, the shapes of this module's adapters) under
        `name` for `forward(..., adapter_rows=)`; the same name again replaces that set in its slot.  Everything is checked
        here, on the host, and the error names the key; the upload into the handle's bank happens at the next forward.  At
        most 64 adapters.  The module's own adapter parameters (what `enable_lora_` set up and training moves) are not
        touched: they serve the calls that pass no `adapter_rows`."""
        if not self.lora_rank:
            raise ValueError("add_adapter: the module has no adapters; call enable_lora_(rank) first")
        if not isinstance(name, str) or not name:
            raise ValueError("add_adapter: the name must be a non-empty string, got %r" % (name,))
        own = dict(self.named_parameters())
        keys = self.lora_keys()
        unknown = sorted(k for k in state_dict if k not in own or "_lora." not in k)
        if unknown:
            raise KeyError("add_adapter(%r): unexpected key '%s' (the accepted keys are lora_keys())" % (name, unknown[0]))
        sd = OrderedDict()
        for k in keys:
            if k not in state_dict:
                raise KeyError("add_adapter(%r): missing key '%s'" % (name, k))
            v = state_dict[k]
            want = tuple(own[k].shape)
            if not torch.is_tensor(v) or v.ndim != 2:
                raise ValueError("add_adapter(%r): '%s' must be a 2-D tensor" % (name, k))
            rank = v.shape[0] if k.endswith("down.weight") else v.shape[1]
            if rank != self.lora_rank:
                raise ValueError("add_adapter(%r): '%s' has rank %d, the module's adapters have rank %d"
                                 % (name, k, rank, self.lora_rank))
            if tuple(v.shape) != want:
                raise ValueError("add_adapter(%r): '%s' has shape %s, expected %s" % (name, k, tuple(v.shape), want))
            sd[k] = v.detach().to(torch.float32).clone()
        slot = self._adapters.get(name)
        if slot is None:
            if len(self._adapters) >= self.ADAPTER_SLOTS_MAX:
                raise ValueError("add_adapter(%r): the bank is full (%d adapters); remove_adapter one first"
                                 % (name, self.ADAPTER_SLOTS_MAX))
            used = set(self._adapters.values())
            slot = next(i for i in range(self.ADAPTER_SLOTS_MAX) if i not in used)
            if slot >= self.adapter_slots:     # a bank is allocated once per handle: a larger one needs a new handle
                self.adapter_slots = min(self.ADAPTER_SLOTS_MAX, max(2 * self.adapter_slots, slot + 1))
                if self._h_bank is not None:
                    self._engine.release()
                    self._h_bank = None
            self._adapters[name] = slot
        self._adapter_ver += 1
        self._slot_state[slot] = (self._adapter_ver, sd)
        return slot

    def adapter_names(self):
        return list(self._adapters)

    def adapter_slot(self, name):
        """The bank slot of a registered adapter: what an int32 device tensor given as `adapter_rows` holds (-1: base)."""
        if name not in self._adapters:
            raise KeyError("unknown adapter %r (registered: %s)" % (name, ", ".join(self._adapters) or "none"))
        return self._adapters[name]

    def remove_adapter(self, name):
        """Forgets `name`; its slot is zeroed at the next forward (a zero adapter is the base model) and free for reuse."""
        slot = self.adapter_slot(name)
        del self._adapters[name]
        self._adapter_ver += 1
        self._slot_state[slot] = (self._adapter_ver, None)

    def _sync_bank(self):
        """Brings the current handle's bank up to the registered adapters: allocates it (a rebuilt handle starts without
        one), then uploads every slot whose contents changed since this handle last saw it."""
        e = self._engine
        if e.h is None or (not self._slot_state and self._h_bank is None):
            return
        L_, dev = N.lib(), self.device
        with torch.cuda.device(dev):
            if self._h_bank is not e.h:
                N.check(L_.ctta_unet_adapter_bank(e.h, int(self.adapter_slots), N.stream_ptr()))
                self._h_bank, self._bank_loaded = e.h, {}
            for slot, (ver, sd) in sorted(self._slot_state.items()):
                have = self._bank_loaded.get(slot)
                if have == ver:
                    continue
                if sd is None and have is None:     # removed before this handle ever loaded it: the slot is still zero
                    self._bank_loaded[slot] = ver
                    continue
                if sd is None:
                    sd = OrderedDict((k, torch.zeros_like(p)) for k, p in self.named_parameters() if "_lora." in k)
                table, keep = N.tensor_table(OrderedDict((k, v.to(dev)) for k, v in sd.items()))
                N.check(L_.ctta_unet_load_adapter_slot(e.h, slot, table, len(table), N.stream_ptr()))
                self._bank_loaded[slot] = ver

    def adapter_row_table(self, batch, adapter_rows, adapter_scales):
        """Host-side check of a call's `adapter_rows` / `adapter_scales` -> (slots, scales): a list of `batch` slot indices
        (-1: base model) or the int32 device tensor as given, and a list of `batch` floats, the float32 device tensor as
        given, or None (every row takes `lora_scale`).  Raises before anything is uploaded; no GPU work."""
        slots = adapter_rows
        if adapter_rows is None:
            slots = [-1] * batch
        elif torch.is_tensor(adapter_rows):
            if adapter_rows.dtype != torch.int32 or adapter_rows.ndim != 1 or adapter_rows.numel() < batch:
                raise ValueError("adapter_rows: a tensor must be 1-D int32 with at least batch = %d entries, got %s %s"
                                 % (batch, adapter_rows.dtype, tuple(adapter_rows.shape)))
            if not adapter_rows.is_cuda:
                raise ValueError("adapter_rows: a tensor of slot indices must live on the device (host callers pass names)")
        else:
            slots = list(adapter_rows)
            if len(slots) != batch:
                raise ValueError("adapter_rows has %d entries, the batch has %d rows" % (len(slots), batch))
            slots = [-1 if n is None else self.adapter_slot(n) for n in slots]
        scales = adapter_scales
        if torch.is_tensor(adapter_scales) and adapter_scales.is_cuda:
            if adapter_scales.dtype != torch.float32 or adapter_scales.ndim != 1 or adapter_scales.numel() < batch:
                raise ValueError("adapter_scales: a tensor must be 1-D float32 with at least batch = %d entries, got %s %s"
                                 % (batch, adapter_scales.dtype, tuple(adapter_scales.shape)))
        elif adapter_scales is not None:
            scales = adapter_scales.tolist() if torch.is_tensor(adapter_scales) else list(adapter_scales)
            if len(scales) != batch:
                raise ValueError("adapter_scales has %d entries, the batch has %d rows" % (len(scales), batch))
            scales = [float(self.lora_scale if s is None else s) for s in scales]
            for i, s in enumerate(scales):
                if not math.isfinite(s):
                    raise ValueError("adapter_scales[%d] = %r is not finite" % (i, s))
        return slots, scales

    def unbind_adapter_rows(self):
        """Back to the single-adapter path, as a `forward` without `adapter_rows` does on its way."""
        if self._bind_adapter_rows(None, None):
            self._text_key = None

    def _bind_adapter_rows(self, slots, scales):
        """Binds (or, both None, unbinds) the row table on the current handle.  True when the rows' adapters may differ
        from the previous forward's -- another mapping, other array contents, a new handle, a bank upload -- so the text
        cache, which holds K / V^T with the adapter terms, must not be reused."""
        e, L_ = self._engine, N.lib()
        if slots is None:
            if self._h_rows is e.h and self._rows_key is not None:
                N.check(L_.ctta_unet_set_adapter_rows(e.h, None, None))
                self._rows_key = self._rows_dev = None
                return True
            self._h_rows = self._rows_key = self._rows_dev = None
            return False
        loaded = dict(self._bank_loaded), self._h_bank
        self._sync_bank()
        if self._h_bank is not e.h:      # no adapter was ever registered: an empty bank, every valid slot is the base model
            with torch.cuda.device(self.device):
                N.check(L_.ctta_unet_adapter_bank(e.h, int(self.adapter_slots), N.stream_ptr()))
            self._h_bank, self._bank_loaded = e.h, {}
        # device arrays by identity + version counter (as the text states; `_rows_dev` keeps them alive), host values by value
        key = tuple((id(v), v._version) if torch.is_tensor(v) else (None if v is None else tuple(v)) for v in (slots, scales))
        changed = loaded != (self._bank_loaded, self._h_bank)
        if self._h_rows is not e.h or key != self._rows_key:
            dev = self.device
            s_dev = slots if torch.is_tensor(slots) else torch.tensor(slots, dtype=torch.int32).to(dev)
            c_dev = scales if scales is None or torch.is_tensor(scales) else torch.tensor(scales, dtype=torch.float32).to(dev)
            N.check(L_.ctta_unet_set_adapter_rows(e.h, N.ptr(s_dev), N.ptr(c_dev)))
            self._h_rows, self._rows_key, self._rows_dev = e.h, key, (s_dev, c_dev)     # the handle reads them: kept alive
            changed = True
        return changed

    def merge_lora_(self):
        """Folds every adapter into its base weight, W += lora_scale * up @ down (fp32, in place; the strength the module
        serves with, 1.0 unless `lora_scale` was set), and drops the adapters: the module is a plain U-Net again and
        serves at the plain U-Net's cost.  `requires_grad` stays as it is (all False)."""
        if not self.lora_rank:
            return self
        params = dict(self.named_parameters())
        with torch.no_grad():
            for key in spec.lora_param_spec(self._cfg, self.lora_rank, self._guided):
                if not key.endswith("down.weight"):
                    continue
                site = key[:-len("down.weight")]                        # "...attn1.processor.to_q_lora."
                attn, layer = site.split("processor.")
                wkey = attn + layer[:-len("_lora.")] + (".0.weight" if layer.startswith("to_out") else ".weight")
                params[wkey].add_(params[site + "up.weight"] @ params[key], alpha=float(self.lora_scale))
        for k, m in list(self.named_modules()):
            if "processor" in m._modules:
                del m._modules["processor"]
        self._frozen_keys = ("guidance_proj.weight",)
        self.lora_rank = 0
        self._adapters.clear()         # the bank goes with the adapters (and with the handle: its key names the rank)
        self._slot_state.clear()
        self._h_bank = self._h_rows = self._rows_key = self._rows_dev = None
        self._drop_flat_()
        return self

    # ---- config plumbing (configuration_utils.py:161,256)
    @classmethod
    def load_config(cls, path, **kwargs):
        with open(path) as f:
            return json.load(f)

    @classmethod
    def from_config(cls, config, subfolder=None, **kwargs):
        return cls(**{k: v for k, v in dict(config).items() if not k.startswith("_")})

    @property
    def device(self):
        return next(self.parameters()).device

    # ---- native handle management
    def _native_config(self, B, H, W, L):
        cfg = self._cfg
        boc, heads, layers = spec.unet_levels(cfg)
        c = N.UNetConfig()
        c.in_channels, c.out_channels, c.n_levels = cfg["in_channels"], cfg["out_channels"], len(boc)
        for i in range(len(boc)):
            c.block_out_channels[i] = boc[i]
            c.heads[i] = heads[i]
            c.layers_per_block[i] = layers[i]
            c.down_cross[i] = int(cfg["down_block_types"][i] == "CrossAttnDownBlock2D")
            c.up_cross[i] = int(cfg["up_block_types"][i] == "CrossAttnUpBlock2D")
        c.cross_attention_dim = cfg["cross_attention_dim"]
        c.norm_num_groups = cfg["norm_num_groups"]
        c.norm_eps = cfg["norm_eps"]
        c.flip_sin_to_cos = int(cfg["flip_sin_to_cos"])
        c.freq_shift = float(cfg["freq_shift"])
        c.guided = int(self._guided)
        c.max_batch, c.height, c.width, c.max_text_len = B, H, W, L
        c.debug_taps = int(self.debug_taps)
        c.enable_training = int(self.enable_training)
        return c

    @property
    def _h_unet(self):
        return self._engine.h

    def _ensure(self, B, H, W, L):
        """Capacity (max_batch, max_text_len) only grows at a fixed (H, W); max_text_len is never below 32 and survives
        an extent change, max_batch does not.  Changed weights are re-packed into the SAME handle."""
        L_, e = N.lib(), self._engine
        key = (H, W, self.debug_taps, self.enable_training, self.device) + ((self.lora_rank,) if self.lora_rank else ())
        ver = self._weights_versions()
        if not e.fits((B, L), key, e.version):
            Bm = max(B, e.capacity[0]) if e.key and e.key[:2] == (H, W) else B
            Lm = max(L, e.capacity[1], 32) if e.key else max(L, 32)
            table, keep = N.tensor_table(self._table())
            cfg = self._native_config(Bm, H, W, Lm)
            e.replace(lambda h: L_.ctta_unet_create(cfg, table, len(table), N.stream_ptr(), h), (Bm, Lm), key, ver,
                      self.device)
        elif ver != e.version:  # parameters changed (optimizer / EMA / load_state_dict)
            if self.lora_rank and isinstance(e.version, tuple) and ver[0] == e.version[0]:
                # only the adapters moved (a LoRA optimizer / EMA step, an adapter-only load_state_dict, a hot swap on a
                # serving module): their 0.1 % of the parameters is re-packed, every base pack stays
                table, keep = N.tensor_table(OrderedDict((k, v) for k, v in self._table().items() if "_lora." in k))
                N.check(L_.ctta_unet_load_adapters(e.h, table, len(table), N.stream_ptr()))
            else:
                table, keep = N.tensor_table(self._table())
                N.check(L_.ctta_unet_load_weights(e.h, table, len(table), N.stream_ptr()))
            e.version = ver

    @staticmethod
    def _per_sample(v, B, device, dtype):
        """_prepare_tensor + expand (unet_2d_condition_guided.py:699-714,803,810)."""
        if not torch.is_tensor(v):
            return torch.full((B,), float(v), dtype=dtype, device=device)
        v = v.to(device=device, dtype=dtype)
        if v.ndim == 0:
            v = v[None]
        return v.expand(B).contiguous()

    def _text_unchanged(self, enc, mask, B, reuse_text):
        """Whether this forward may take the cross-attention K / V projections of the text states from the handle's text
        cache (ctta_unet_reuse_text): the SAME tensor objects as in the previous forward on this module, unmodified since
        (identity + version counters; the module keeps a reference, so the storage cannot have been recycled).  Inside a
        hipGraph capture only on the caller's explicit word (`reuse_text=True`): a replay cannot re-decide."""
        key = (enc, enc._version, mask, None if mask is None else mask._version, B)
        prev = getattr(self, "_text_key", None)
        same = (prev is not None and prev[0] is key[0] and prev[1] == key[1] and prev[2] is key[2] and prev[3] == key[3]
                and prev[4] == key[4])
        # the key of THIS forward is committed by `_forward` after the native call has returned OK (a failed forward must
        # not leave its text states registered as "the cached ones").  Identity + `_version` cannot see writes through raw
        # pointers (how this library's own kernels fill tensors): a caller that refills a persistent text-state buffer
        # natively must pass reuse_text=False.
        self._text_key_pending = key
        if reuse_text is False or not same:
            return False
        if reuse_text is True:
            return True
        return not torch.cuda.is_current_stream_capturing()

    @staticmethod
    def _call_lora_scale(cross_attention_kwargs):
        """diffusers' `cross_attention_kwargs={"scale": s}` (LoRAAttnProcessor.__call__(..., scale=)): the adapter strength
        of THIS call, or None.  Nothing else travels through that dict here."""
        if not cross_attention_kwargs:
            return None
        unknown = sorted(k for k in cross_attention_kwargs if k != "scale")
        if unknown:
            raise NotImplementedError("cross_attention_kwargs %s: only 'scale' (the LoRA strength) is supported" % unknown)
        return float(cross_attention_kwargs["scale"])

    def _forward(self, sample, timestep, guidance, encoder_hidden_states, encoder_attention_mask, train=False,
                 reuse_text=None, lora_scale=None, adapter_rows=None, adapter_scales=None):
        if sample.ndim != 4 or sample.shape[1] != self._cfg["in_channels"]:
            raise ValueError("sample must be (batch, %d, height, width), got %s"
                             % (self._cfg["in_channels"], tuple(sample.shape)))
        if encoder_hidden_states is None or encoder_hidden_states.ndim != 3:
            raise ValueError("encoder_hidden_states must be (batch, sequence_length, feature_dim)")
        B, _, H, W = sample.shape
        L = encoder_hidden_states.shape[1]
        if encoder_hidden_states.shape[0] != B or encoder_hidden_states.shape[2] != self._cfg["cross_attention_dim"]:
            raise ValueError("encoder_hidden_states shape %s does not match batch %d / cross_attention_dim %d"
                             % (tuple(encoder_hidden_states.shape), B, self._cfg["cross_attention_dim"]))
        slots = scales = None
        if adapter_rows is not None or adapter_scales is not None:     # checked on the host before anything is uploaded
            if not self.lora_rank:
                raise ValueError("adapter_rows / adapter_scales: the module has no adapters; call enable_lora_(rank) first")
            if train:
                raise ValueError("forward_train takes no adapter_rows: training mixes no adapters")
            slots, scales = self.adapter_row_table(B, adapter_rows, adapter_scales)
        dev = self.device
        if not sample.is_cuda:
            raise N.CttaError("sample is on %s: the HIP engine has no CPU path" % sample.device)
        had_handle, ver0 = self._h_unet is not None, self._engine.version
        self._ensure(B, H, W, L)
        # a training forward leaves the binding alone: with rows bound the handle refuses it (unbind_adapter_rows first)
        if not train and self._bind_adapter_rows(slots, scales):
            self._text_key = None      # the cached K / V^T hold the previous mapping's adapter terms
        reuse = self._text_unchanged(encoder_hidden_states, encoder_attention_mask, B, reuse_text)
        reuse = reuse and not train and had_handle and ver0 == self._engine.version  # same handle, same packed weights
        x = sample.detach().to(device=dev, dtype=torch.float32).contiguous()
        enc = encoder_hidden_states.detach().to(device=dev, dtype=torch.float32).contiguous()
        t = self._per_sample(timestep, B, dev, torch.float32)  # get_timestep_embedding casts to fp32
        g = self._per_sample(guidance, B, dev, torch.float64) if self._guided else None
        m = None
        if encoder_attention_mask is not None:
            m = encoder_attention_mask.to(device=dev).reshape(B, L).to(torch.uint8).contiguous()
        out = torch.empty((B, self._cfg["out_channels"], H, W), dtype=torch.float32, device=dev)
        fn = N.lib().ctta_unet_forward_train if train else N.lib().ctta_unet_forward
        self._text_key = None
        with torch.cuda.device(dev):
            if self.lora_rank:   # a changed scale drops the handle's text cache (it holds the adapter term)
                N.check(N.lib().ctta_unet_set_lora(self._h_unet, int(self.lora_fused),
                                                   float(self.lora_scale if lora_scale is None else lora_scale)))
            if reuse:
                N.check(N.lib().ctta_unet_reuse_text(self._h_unet, 1))
            N.check(fn(self._h_unet, N.ptr(x), N.ptr(t), N.ptr(g), N.ptr(enc), N.ptr(m), B, L, N.ptr(out),
                       N.stream_ptr()))
        self._text_key = getattr(self, "_text_key_pending", None)
        return out

    # ---- distillation step: the reference differentiates `forward` with torch autograd
    # (train.py:332-346); here the engine keeps the activations and runs its own backward pass.
    def forward_train(self, sample, timestep, guidance, encoder_hidden_states, encoder_attention_mask=None):
        """`forward` that keeps what `backward` needs.  Returns the prediction (B,C,H,W) fp32, detached."""
        if not self.enable_training:
            self.enable_training = True
        return self._forward(sample, timestep, guidance if self._guided else None, encoder_hidden_states,
                             encoder_attention_mask, train=True)

    def backward(self, grad_output=None, grad_output_nhwc=None, on_block_done=None):
        """Accumulates dL/d(param) of the last `forward_train` into `p.grad` (fp32, allocated on first
        use).  `grad_output`: dL/d(prediction) (B,C,H,W) fp32, or `grad_output_nhwc`: the same as the
        (B, H*W, 8) bf16 tensor ctta_snr_mse_grad writes."""
        dev = self.device
        if grad_output_nhwc is None:
            B, C, H, W = grad_output.shape
            g = torch.zeros(B, H * W, 8, dtype=torch.bfloat16, device=dev)
            g[:, :, :C] = grad_output.detach().to(dev).permute(0, 2, 3, 1).reshape(B, H * W, C).to(torch.bfloat16)
            grad_output_nhwc = g
        tab, keep = self._grad_table()
        g = grad_output_nhwc.contiguous()
        with torch.cuda.device(dev):
            if on_block_done is None:
                N.check(N.lib().ctta_unet_backward(self._h_unet, N.ptr(g), tab, len(tab), N.stream_ptr()))
                return
        # block-wise: after each step the gradients of one block are final; the callback typically starts
        # the all-reduce of that block's slice of the flat gradient buffer (dist_util.GradientBuckets)
        on_block_done(self.backward_begin(g))
        fin = False
        while not fin:
            blk, fin = self.backward_next()
            on_block_done(blk)

    def _grad_table(self):
        table = OrderedDict()
        if getattr(self, "_flat_grad", None) is not None and not self.grads_alias_flat():
            self.realias_grads_()    # e.g. after zero_grad(set_to_none=True): the fused optimizer reads the flat buffer
        for k, p in self.named_parameters():
            if not p.requires_grad:
                continue
            if p.grad is None:
                p.grad = torch.zeros_like(p.data)
            table[k] = p.grad
        return N.tensor_table(table)

    def backward_begin(self, grad_output_nhwc):
        """First step of the block-wise backward (ctta_unet_backward_begin): the out head.  Returns its block id.  Each
        begin / next call is self-contained on the calling stream (the weight-gradient side stream is joined before it
        returns), so a caller may capture every call into its own hipGraph (`_DistillStepGraph(segmented=True)`)."""
        tab, keep = self._bwd_table = self._grad_table()     # kept for the `backward_next` calls of THIS backward pass
        with torch.cuda.device(self.device):
            N.check(N.lib().ctta_unet_backward_begin(self._h_unet, N.ptr(grad_output_nhwc), tab, len(tab), N.stream_ptr()))
        return 2 * len(self._cfg["block_out_channels"]) + 2

    def backward_next(self):
        """One more block (ctta_unet_backward_next) -> (block id, finished)."""
        # the table `backward_begin` built (690 named gradient tensors: rebuilding it for each of the ~12 calls of one
        # block-wise backward was host time on the data-parallel step's critical path; the gradient tensors cannot change
        # between the calls of one pass)
        tab, keep = getattr(self, "_bwd_table", None) or self._grad_table()
        blk, fin = N.c_int(0), N.c_int(0)
        with torch.cuda.device(self.device):
            N.check(N.lib().ctta_unet_backward_next(self._h_unet, tab, len(tab), N.stream_ptr(), N.byref(blk), N.byref(fin)))
        if fin.value:
            self._bwd_table = None
        return blk.value, bool(fin.value)

    def block_ranges(self):
        """block id (see ctta_unet_backward_next) -> (start, end) element range of that block's parameters in the
        flat parameter / gradient buffers (trainable parameters only; state-dict order keeps blocks contiguous)."""
        n_levels = len(self._cfg["block_out_channels"])

        def block_of(key):
            head, _, rest = key.partition(".")
            if head == "down_blocks":
                return 1 + int(rest.split(".")[0])
            if head == "mid_block":
                return 1 + n_levels
            if head == "up_blocks":
                return 2 + n_levels + int(rest.split(".")[0])
            if head in ("conv_norm_out", "conv_out"):
                return 2 * n_levels + 2
            return 0   # conv_in, time_embedding, guidance_embedding
        frozen = set(getattr(self, "_frozen_keys", ()))
        ranges, off = {}, 0
        for k, p in self.named_parameters():
            if k in frozen:
                continue
            b = block_of(k)
            lo, hi = ranges.get(b, (off, off))
            if hi != off:
                raise RuntimeError("parameters of block %d are not contiguous in the flat buffer" % b)
            ranges[b] = (lo, off + p.numel())
            off += p.numel()
        return ranges

    def read_taps(self):
        """name -> NCHW fp32 tensor of every recorded intermediate (debug_taps=True only)."""
        return N.read_taps("ctta_unet", self._h_unet, self.device)


class UNet2DConditionGuidedModel(_UNetBase):
    """Student / consistency U-Net with the guidance-strength Fourier input."""
    _guided = True

    def forward(self, sample, timestep, guidance, encoder_hidden_states, class_labels=None, timestep_cond=None,
                guidance_cond=None, attention_mask=None, cross_attention_kwargs=None, added_cond_kwargs=None,
                down_block_additional_residuals=None, mid_block_additional_residual=None,
                encoder_attention_mask=None, return_dict=True, adapter_rows=None, adapter_scales=None, **kwargs):
        for name, v in (("class_labels", class_labels), ("timestep_cond", timestep_cond),
                        ("guidance_cond", guidance_cond), ("attention_mask", attention_mask),
                        ("down_block_additional_residuals", down_block_additional_residuals),
                        ("mid_block_additional_residual", mid_block_additional_residual)):
            if v is not None:
                raise NotImplementedError("%s is not used on the ConsistencyTTA path and is not supported" % name)
        out = self._forward(sample, timestep, guidance, encoder_hidden_states, encoder_attention_mask,
                            reuse_text=kwargs.get("reuse_text"), lora_scale=self._call_lora_scale(cross_attention_kwargs),
                            adapter_rows=adapter_rows, adapter_scales=adapter_scales)
        return UNet2DConditionOutput(sample=out) if return_dict else (out,)


class UNet2DConditionModel(_UNetBase):
    """Teacher diffusion U-Net; `forward(**kwargs)` swallows `guidance=` like the reference
    (unet_2d_condition.py:668-690)."""
    _guided = False

    def forward(self, sample, timestep, encoder_hidden_states, class_labels=None, timestep_cond=None,
                attention_mask=None, cross_attention_kwargs=None, added_cond_kwargs=None,
                down_block_additional_residuals=None, mid_block_additional_residual=None,
                encoder_attention_mask=None, return_dict=True, adapter_rows=None, adapter_scales=None, **kwargs):
        out = self._forward(sample, timestep, None, encoder_hidden_states, encoder_attention_mask,
                            reuse_text=kwargs.get("reuse_text"), lora_scale=self._call_lora_scale(cross_attention_kwargs),
                            adapter_rows=adapter_rows, adapter_scales=adapter_scales)
        return UNet2DConditionOutput(sample=out) if return_dict else (out,)


# ------------------------------------------------------------------------------------------
class DiagonalGaussianDistribution(object):
    """audioldm/variational_autoencoder/distributions.py:24-74 (elementwise torch ops on the moments the HIP
    encoder produced; sampling draws from the global RNG exactly like the reference)."""

    def __init__(self, parameters, deterministic=False):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.deterministic = deterministic
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)
        if self.deterministic:
            self.var = self.std = torch.zeros_like(self.mean).to(device=self.parameters.device)

    def sample(self):
        return self.mean + self.std * torch.randn(self.mean.shape).to(device=self.parameters.device)

    def kl(self, other=None):
        if self.deterministic:
            return torch.Tensor([0.0])
        if other is None:
            return 0.5 * torch.mean(torch.pow(self.mean, 2) + self.var - 1.0 - self.logvar, dim=[1, 2, 3])
        return 0.5 * torch.mean(torch.pow(self.mean - other.mean, 2) / other.var + self.var / other.var - 1.0
                                - self.logvar + other.logvar, dim=[1, 2, 3])

    def mode(self):
        return self.mean


class _VaeDecodeWithGrad(torch.autograd.Function):
    """decode_first_stage under torch.set_grad_enabled(True) (autoencoder.py:103-106) for a frozen decoder: the HIP
    engine keeps its own saved tensors between the two calls; one forward may be pending per AutoencoderKL."""

    @staticmethod
    def forward(ctx, z, vae):
        B, _, T, F = z.shape
        h = vae._ensure_vae(B, T, F, grad=True)
        zz = z.detach().to(device=vae.device, dtype=torch.float32).contiguous()
        up = 2 ** (len(vae.ddconfig["ch_mult"]) - 1)
        mel = torch.empty((B, vae.ddconfig["out_ch"], T * up, F * up), dtype=torch.float32, device=vae.device)
        with torch.cuda.device(vae.device):
            N.check(N.lib().ctta_vae_decode_with_grad(h, N.ptr(zz), B, N.ptr(mel), N.stream_ptr()))
        ctx.vae, ctx.shape, ctx.dtype = vae, tuple(z.shape), z.dtype
        ctx.token = vae._vae_pending = object()
        return mel

    @staticmethod
    def backward(ctx, grad_mel):
        vae = ctx.vae
        if vae._vae_pending is not ctx.token:
            raise N.CttaError("decode_first_stage(allow_grad=True): the decoder ran again (or its handle was rebuilt) "
                              "before this backward -- only the latest differentiable decode can be back-propagated")
        g = grad_mel.to(device=vae.device, dtype=torch.float32).contiguous()
        gz = torch.empty(ctx.shape, dtype=torch.float32, device=vae.device)
        with torch.cuda.device(vae.device):
            N.check(N.lib().ctta_vae_decode_backward(vae._eng["vae"][1].h, N.ptr(g), ctx.shape[0], N.ptr(gz), N.stream_ptr()))
        vae._vae_pending = None
        return gz.to(ctx.dtype), None


class _VaeDecodeWithParamGrad(torch.autograd.Function):
    """decode_first_stage(allow_grad=True) for a TRAINABLE decoder (AudioLCM_FTVAE): the backward also accumulates
    d loss / d parameter of every decoder.* / post_quant_conv.* tensor into the `.grad` views of the VAE's flat gradient
    buffer (ctta_vae_decode_backward_params).  `anchor` is a scalar that requires grad, so that the backward runs even when
    the latent itself does not require grad (the pattern of models._EngineLoss)."""

    @staticmethod
    def forward(ctx, z, anchor, vae):
        B, _, T, F = z.shape
        h = vae._ensure_vae(B, T, F, grad=2)
        zz = z.detach().to(device=vae.device, dtype=torch.float32).contiguous()
        up = 2 ** (len(vae.ddconfig["ch_mult"]) - 1)
        mel = torch.empty((B, vae.ddconfig["out_ch"], T * up, F * up), dtype=torch.float32, device=vae.device)
        with torch.cuda.device(vae.device):
            N.check(N.lib().ctta_vae_decode_with_grad(h, N.ptr(zz), B, N.ptr(mel), N.stream_ptr()))
        ctx.vae, ctx.shape, ctx.dtype, ctx.need_z = vae, tuple(z.shape), z.dtype, z.requires_grad
        ctx.token = vae._vae_pending = object()
        return mel

    @staticmethod
    def backward(ctx, grad_mel):
        vae = ctx.vae
        if vae._vae_pending is not ctx.token:
            raise N.CttaError("decode_first_stage(allow_grad=True): the decoder ran again (or its handle was rebuilt) "
                              "before this backward -- only the latest differentiable decode can be back-propagated")
        g = grad_mel.to(device=vae.device, dtype=torch.float32).contiguous()
        gz = torch.empty(ctx.shape, dtype=torch.float32, device=vae.device) if ctx.need_z else None
        vae.flat_grad_()
        if not vae.grads_alias_flat():
            vae.realias_grads_()
        table, keep = N.tensor_table({k: p.grad for k, p in vae._decoder_named()})
        with torch.cuda.device(vae.device):
            N.check(N.lib().ctta_vae_decode_backward_params(vae._eng["vae"][1].h, N.ptr(g), ctx.shape[0], N.ptr(gz), table,
                                                            len(table), N.stream_ptr()))
        vae._vae_pending = None
        return (gz.to(ctx.dtype) if ctx.need_z else None), None, None


class _DecoderShadow(_ParamTree):
    """Frozen parameter holder with the decoder's (or post_quant_conv's) own key names: the EMA copies of AudioLCM_FTVAE
    (audio_consistency_model_ftvae.py:52-57)."""

    def __init__(self, table):
        super().__init__()
        self._register(table, frozen=tuple(table))
        self.eval()


class _VocodeWithGrad(torch.autograd.Function):
    """vocoder(mels) of vocoder_infer(allow_grad=True) (hifigan/utilities.py:79-80) for the frozen generator."""

    @staticmethod
    def forward(ctx, mel, vae):
        if mel.ndim != 4 or mel.shape[1] != 1 or mel.shape[3] != vae.vocoder.h["num_mels"]:
            raise ValueError("mel must be (batch, 1, T, %d), got %s" % (vae.vocoder.h["num_mels"], tuple(mel.shape)))
        if not mel.is_cuda:
            raise N.CttaError("mel is on %s: the HIP engine has no CPU path" % mel.device)
        B, _, T, F = mel.shape
        h = vae._ensure_voc(B, T, grad=True)
        m = mel.detach().to(device=vae.device, dtype=torch.float32).contiguous()
        n = N.lib().ctta_hifigan_out_len(h, T)
        wav = torch.empty((B, n), dtype=torch.float32, device=vae.device)
        with torch.cuda.device(vae.device):
            N.check(N.lib().ctta_hifigan_forward_with_grad(h, N.ptr(m), B, T, N.ptr(wav), N.stream_ptr()))
        ctx.vae, ctx.shape, ctx.dtype = vae, tuple(mel.shape), mel.dtype
        ctx.token = vae._voc_pending = object()
        ctx.save_for_backward(wav)
        return wav

    @staticmethod
    def backward(ctx, grad_wav):
        vae = ctx.vae
        if vae._voc_pending is not ctx.token:
            raise N.CttaError("decode_to_waveform(allow_grad=True): the vocoder ran again (or its handle was rebuilt) "
                              "before this backward -- only the latest differentiable call can be back-propagated")
        (wav,) = ctx.saved_tensors
        B, _, T, F = ctx.shape
        g = grad_wav.to(device=vae.device, dtype=torch.float32).contiguous()
        gm = torch.empty(ctx.shape, dtype=torch.float32, device=vae.device)
        with torch.cuda.device(vae.device):
            N.check(N.lib().ctta_hifigan_backward(vae._eng["voc"][1].h, N.ptr(g), N.ptr(wav), B, T, N.ptr(gm), N.stream_ptr()))
        vae._voc_pending = None
        return gm.to(ctx.dtype), None


class Generator(_ParamTree):
    """HiFi-GAN parameter holder (weight_norm already removed, hifigan/utilities.py:71)."""

    def __init__(self, h=None):
        super().__init__()
        self.h = dict(spec.HIFIGAN_16K_64 if h is None else h)
        self._register(spec.hifigan_param_spec(self.h, prefix=""))


class AutoencoderKL(_ParamTree):
    """AudioLDM VAE (autoencoder.py:10-132): `decode_first_stage` / `decode_to_waveform` (generation) and
    `encode_first_stage` / `get_first_stage_encoding` (the training-side latent encoder, tools/train_utils.py:155-162)."""

    def __init__(self, ddconfig=None, lossconfig=None, image_key="fbank", embed_dim=None, time_shuffle=1,
                 subband=1, ckpt_path=None, reload_from_ckpt=None, ignore_keys=(), colorize_nlabels=None,
                 monitor=None, base_learning_rate=1e-5, scale_factor=1, hifigan_config=None, **ignored):
        super().__init__()
        self.ddconfig = dict(spec.VAE_DDCONFIG if ddconfig is None else ddconfig)
        self.embed_dim = int(embed_dim if embed_dim is not None else 8)
        if int(subband) != 1:
            raise NotImplementedError("subband decomposition is unused by ConsistencyTTA (subband=1)")
        if self.ddconfig.get("attn_resolutions"):
            raise NotImplementedError("attn_resolutions must be empty (audioldm-s-full)")
        self.subband = 1
        self.image_key = image_key
        self.scale_factor = scale_factor
        # reference state-dict order: encoder.*, decoder.*, quant_conv.*, post_quant_conv.*, vocoder.*
        enc = spec.vae_encoder_param_spec(self.ddconfig, self.embed_dim)
        dec = spec.vae_decoder_param_spec(self.ddconfig, self.embed_dim)
        table = OrderedDict((k, v) for k, v in enc.items() if k.startswith("encoder."))
        table.update((k, v) for k, v in dec.items() if k.startswith("decoder."))
        table.update((k, v) for k, v in enc.items() if k.startswith("quant_conv."))
        table.update((k, v) for k, v in dec.items() if k.startswith("post_quant_conv."))
        self._register(table)
        self.vocoder = Generator(hifigan_config)
        self._enc = N.EngineHandle("ctta_vae_encoder_destroy")
        self.ema_decoder = self.ema_post_quant_conv = None     # set by AudioLCM_FTVAE (autoencoder.py:91-101 decodes through them)
        self._ema_eng = N.EngineHandle("ctta_vae_destroy")
        # engine handles: [plain, differentiable] per stage -- separate handles, so that a plain decode (e.g. of the
        # target latent in MelLoss) never disturbs the tensors a pending differentiable decode saved for its backward
        self._eng = {"vae": [N.EngineHandle("ctta_vae_destroy") for _ in range(2)],
                     "voc": [N.EngineHandle("ctta_hifigan_destroy") for _ in range(2)]}
        self._h_vae = self._h_voc = None     # the handle each stage used last (debug taps)
        self._vae_pending = self._voc_pending = None
        self.debug_taps = False

    @property
    def device(self):
        return next(self.parameters()).device

    def load_state_dict(self, state_dict, strict=True):
        """Reference checkpoints also carry loss.* (discriminator) and ema_* keys, which this path never uses.
        A decoder-only state dict (generation checkpoints without the encoder) loads too: missing encoder.* /
        quant_conv.* keys are tolerated and `encode*` then raises until they are provided."""
        own = {k: v for k, v in state_dict.items() if not k.startswith(("loss.", "ema_"))}
        has_enc = any(k.startswith("encoder.") for k in own)
        self._encoder_loaded = has_enc or getattr(self, "_encoder_loaded", False)
        if not has_enc:
            mine = self.state_dict()
            own.update({k: v for k, v in mine.items() if k.startswith(("encoder.", "quant_conv."))})
        return super().load_state_dict(own, strict=strict)

    def init_deterministic(self, seed=0, prefix=""):
        self._encoder_loaded = True
        return super().init_deterministic(seed, prefix)

    def init_random_(self, seed=0, prefix=""):
        self._encoder_loaded = True
        return super().init_random_(seed, prefix)

    # ---- encoder, autoencoder.py:80-89,123-132
    def _ensure_enc(self, B, T, F):
        L_ = N.lib()
        nres = len(self.ddconfig["ch_mult"])
        s = 1 << (nres - 1)
        if T % s or F % s:
            raise ValueError("mel extent %dx%d must be a multiple of %d" % (T, F, s))
        key = (T, F, self.debug_taps, self.device)
        named = [(k, p) for k, p in self.named_parameters() if k.startswith(("encoder.", "quant_conv."))]
        ver = sum(p._version for k, p in named)
        if not self._enc.fits((B,), key, ver):
            dd = self.ddconfig
            c = N.VAEConfig()
            c.z_channels, c.embed_dim, c.ch, c.out_ch = dd["z_channels"], self.embed_dim, dd["ch"], dd["in_channels"]
            c.n_levels, c.num_res_blocks = nres, dd["num_res_blocks"]
            for i, m in enumerate(dd["ch_mult"]):
                c.ch_mult[i] = m
            c.scale_factor = float(self.scale_factor)
            c.max_batch, c.latent_h, c.latent_w = B, T // s, F // s
            c.debug_taps = int(self.debug_taps)
            table, keep = N.param_table(named)
            self._enc.replace(lambda h: L_.ctta_vae_encoder_create(c, table, len(table), N.stream_ptr(), h), (B,), key, ver,
                              self.device)
        return self._enc.h

    @torch.no_grad()
    def encode(self, x):
        """mel (B,1,T,F) -> DiagonalGaussianDistribution over the latent (B, embed_dim, T/4, F/4)."""
        if not getattr(self, "_encoder_loaded", False):
            raise RuntimeError("this AutoencoderKL was loaded from a decoder-only state dict: no encoder weights")
        if x.ndim != 4 or x.shape[1] != self.ddconfig["in_channels"]:
            raise ValueError("mel must be (batch, %d, T, F), got %s" % (self.ddconfig["in_channels"], tuple(x.shape)))
        if not x.is_cuda:
            raise N.CttaError("mel is on %s: the HIP engine has no CPU path" % x.device)
        B, _, T, F = x.shape
        h = self._ensure_enc(B, T, F)
        s = 1 << (len(self.ddconfig["ch_mult"]) - 1)
        mel = x.detach().to(device=self.device, dtype=torch.float32).contiguous()
        moments = torch.empty((B, 2 * self.embed_dim, T // s, F // s), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            N.check(N.lib().ctta_vae_encode(h, N.ptr(mel), B, N.ptr(moments), N.stream_ptr()))
        return DiagonalGaussianDistribution(moments)

    encode_first_stage = encode

    def get_first_stage_encoding(self, encoder_posterior):
        if isinstance(encoder_posterior, DiagonalGaussianDistribution):
            z = encoder_posterior.sample()
        elif isinstance(encoder_posterior, torch.Tensor):
            z = encoder_posterior
        else:
            raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")
        return self.scale_factor * z

    def read_encoder_taps(self):
        return N.read_taps("ctta_vae_encoder", self._enc.h, self.device)

    _DECODER_KEYS = ("decoder.", "post_quant_conv.")

    def _decoder_named(self):
        return [(k, p) for k, p in self.named_parameters() if k.startswith(self._DECODER_KEYS)]

    def decoder_trainable(self):
        return any(p.requires_grad for _, p in self._decoder_named())

    def train_decoder_(self, mode=True):
        """Fine-tuning of the decoder (audio_consistency_model_ftvae.py:59-62): decoder.* and post_quant_conv.* require grad
        and become the trainable PREFIX of the flat parameter / gradient buffers -- what `optim.FusedAdamW(vae)` and the EMA
        kernel run over; encoder, quant_conv and vocoder stay frozen behind it."""
        self._decoder_training = bool(mode)
        frozen = tuple(k for k, _ in self.named_parameters() if not (mode and k.startswith(self._DECODER_KEYS)))
        for k, p in self.named_parameters():
            p.requires_grad_(bool(mode) and k.startswith(self._DECODER_KEYS))
            if not p.requires_grad:
                p.grad = None
        if frozen != tuple(getattr(self, "_frozen_keys", ())):
            self._frozen_keys = frozen
            self._flat = self._flat_grad = None      # the flat order changed: the next flatten_parameters_() re-homes
            self._trainable_cache = None
        return self

    def _make_config(self, B, T, F, sf, grad):
        dd = self.ddconfig
        c = N.VAEConfig()
        c.z_channels, c.embed_dim, c.ch, c.out_ch = dd["z_channels"], self.embed_dim, dd["ch"], dd["out_ch"]
        c.n_levels, c.num_res_blocks = len(dd["ch_mult"]), dd["num_res_blocks"]
        for i, m in enumerate(dd["ch_mult"]):
            c.ch_mult[i] = m
        c.scale_factor = sf
        c.max_batch, c.latent_h, c.latent_w = B, T, F
        c.debug_taps = int(self.debug_taps)
        c.enable_grad = int(grad)
        return c

    def _ensure_ema_vae(self, B, T, F):
        """Plain handle over the EMA decoder / post_quant_conv holders (decode_first_stage(use_ema=True))."""
        L_ = N.lib()
        sf = float(self.scale_factor)
        key = (T, F, sf, self.device)
        named = [("decoder." + k, p) for k, p in self.ema_decoder.named_parameters()]
        named += [("post_quant_conv." + k, p) for k, p in self.ema_post_quant_conv.named_parameters()]
        ver = (sum(p._version for _, p in named) + 7 * getattr(self.ema_decoder, "_manual_version", 0)
               + 7 * getattr(self.ema_post_quant_conv, "_manual_version", 0))
        e = self._ema_eng
        if not e.fits((B,), key, ver):
            table, keep = N.param_table(named)
            if e.h is not None and e.key == key and B <= e.capacity[0]:
                with torch.cuda.device(self.device):
                    N.check(L_.ctta_vae_load_weights(e.h, table, len(table), N.stream_ptr()))
                e.version = ver
            else:
                c = self._make_config(B, T, F, sf, 0)
                e.replace(lambda h: L_.ctta_vae_create(c, table, len(table), N.stream_ptr(), h), (B,), key, ver, self.device)
        return e.h

    def _ensure_vae(self, B, T, F, grad=False):
        """grad: 0 plain, 1 differentiable in z (frozen decoder), 2 parameter gradients as well (trainable decoder)."""
        L_ = N.lib()
        sf = float(self.scale_factor)
        key = (T, F, sf, self.debug_taps, self.device) + ((2,) if int(grad) == 2 else ())
        named = self._decoder_named()
        training = getattr(self, "_decoder_training", False)       # train_decoder_(): the weights move every step
        # the fused optimizer updates a trainable decoder through raw pointers: mark_weights_changed() counts those
        ver = sum(p._version for k, p in named) + (7 * getattr(self, "_manual_version", 0) if training else 0)
        e = self._eng["vae"][int(bool(grad))]
        if training and e.h is not None and e.key == key and B <= e.capacity[0] and e.version != ver:
            # an optimizer step moved the weights: repack them in place instead of rebuilding the handle
            table, keep = N.param_table(named)
            with torch.cuda.device(self.device):
                N.check(L_.ctta_vae_load_weights(e.h, table, len(table), N.stream_ptr()))
            e.version = ver
            if grad:
                self._vae_pending = None
        if not e.fits((B,), key, ver):
            c = self._make_config(B, T, F, sf, grad)
            if grad:
                self._vae_pending = None
            table, keep = N.param_table(named)
            e.replace(lambda h: L_.ctta_vae_create(c, table, len(table), N.stream_ptr(), h), (B,), key, ver, self.device)
        self._h_vae = e.h
        return e.h

    def _ensure_voc(self, B, frames, grad=False):
        L_ = N.lib()
        named = [("vocoder." + k, p) for k, p in self.vocoder.named_parameters()]
        ver = sum(p._version for k, p in named)
        key = (self.debug_taps, self.device)
        e = self._eng["voc"][int(grad)]
        if not e.fits((B, frames), key, ver):
            h_ = self.vocoder.h
            c = N.HifiganConfig()
            c.num_mels, c.upsample_initial_channel = h_["num_mels"], h_["upsample_initial_channel"]
            c.n_ups, c.n_kernels = len(h_["upsample_rates"]), len(h_["resblock_kernel_sizes"])
            for i, (u, k) in enumerate(zip(h_["upsample_rates"], h_["upsample_kernel_sizes"])):
                c.upsample_rates[i], c.upsample_kernel_sizes[i] = u, k
            for j, (k, dil) in enumerate(zip(h_["resblock_kernel_sizes"], h_["resblock_dilation_sizes"])):
                c.resblock_kernel_sizes[j] = k
                for m in range(3):
                    c.resblock_dilations[j][m] = dil[m]
            c.max_batch, c.max_frames, c.debug_taps = B, frames, int(self.debug_taps)
            c.enable_grad = int(grad)
            if grad:
                self._voc_pending = None
            table, keep = N.param_table(named)
            e.replace(lambda h: L_.ctta_hifigan_create(c, table, len(table), N.stream_ptr(), h), (B, frames), key, ver,
                      self.device)
        self._h_voc = e.h
        return e.h

    # ---- reference API
    def decode(self, z, use_ema=False):
        return self.decode_first_stage(z * self.scale_factor, use_ema=use_ema)

    def decode_first_stage(self, z, allow_grad=False, use_ema=False):
        """z (B,8,T,F) -> mel (B,1,4T,4F); z is divided by scale_factor first (autoencoder.py:105).
        allow_grad=True (CLAPLoss, tools/losses.py:294-296) returns a mel that back-propagates into z through the
        frozen decoder (ctta_vae_decode_with_grad / ctta_vae_decode_backward).  When decoder.* / post_quant_conv.* require
        grad (`train_decoder_()`, AudioLCM_FTVAE) the backward also accumulates their gradients, whether or not z requires
        grad.  use_ema=True decodes through `ema_decoder` / `ema_post_quant_conv` when they are set (autoencoder.py:91-101)."""
        if use_ema and self.ema_decoder is None:
            print("VAE does not have EMA modules, but specified use_ema. Using the none-EMA modules instead.")
        if z.ndim != 4 or z.shape[1] != self.embed_dim:
            raise ValueError("z must be (batch, %d, T, F), got %s" % (self.embed_dim, tuple(z.shape)))
        if not z.is_cuda:
            raise N.CttaError("z is on %s: the HIP engine has no CPU path" % z.device)
        ema = use_ema and self.ema_decoder is not None
        if allow_grad and torch.is_grad_enabled() and not ema and self.decoder_trainable():
            if not all(p.requires_grad for _, p in self._decoder_named()):
                raise N.CttaError("decode_first_stage(allow_grad=True): only some decoder parameters require grad -- "
                                  "train_decoder_() makes decoder.* and post_quant_conv.* trainable together")
            return _VaeDecodeWithParamGrad.apply(z, self._grad_anchor(), self)
        if allow_grad and torch.is_grad_enabled() and z.requires_grad and not ema:
            return _VaeDecodeWithGrad.apply(z, self)
        B, _, T, F = z.shape
        h = self._ensure_ema_vae(B, T, F) if ema else self._ensure_vae(B, T, F)
        zz = z.detach().to(device=self.device, dtype=torch.float32).contiguous()
        up = 2 ** (len(self.ddconfig["ch_mult"]) - 1)
        mel = torch.empty((B, self.ddconfig["out_ch"], T * up, F * up), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            N.check(N.lib().ctta_vae_decode(h, N.ptr(zz), B, N.ptr(mel), N.stream_ptr()))
        return mel

    def _grad_anchor(self):
        a = getattr(self, "_anchor", None)
        if a is None or a.device != self.device:
            a = self._anchor = torch.zeros((), device=self.device, requires_grad=True)
        return a

    def vocode(self, mel):
        """mel (B,1,T,F) -> float waveform (B, L) before centring (Generator.forward)."""
        if mel.ndim != 4 or mel.shape[1] != 1 or mel.shape[3] != self.vocoder.h["num_mels"]:
            raise ValueError("mel must be (batch, 1, T, %d), got %s" % (self.vocoder.h["num_mels"], tuple(mel.shape)))
        if not mel.is_cuda:
            raise N.CttaError("mel is on %s: the HIP engine has no CPU path" % mel.device)
        B, _, T, F = mel.shape
        h = self._ensure_voc(B, T)
        m = mel.detach().to(device=self.device, dtype=torch.float32).contiguous()
        n = N.lib().ctta_hifigan_out_len(h, T)
        wav = torch.empty((B, n), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            N.check(N.lib().ctta_hifigan_forward(h, N.ptr(m), B, T, N.ptr(wav), N.stream_ptr()))
        return wav

    def decode_to_waveform(self, dec, allow_grad=False, return_float=False, world_extrema=False):
        """vocoder_infer (hifigan/utilities.py:76-91): batch-global (max+min)/2 centring, then
        int16 numpy on the host (the reference's return type); return_float keeps the centred
        float tensor on the device.  allow_grad=True returns the centred float waveform with a graph back to `dec`
        (utilities.py:79-81; the centring's max/min run as torch ops on the vocoder's differentiable output).
        world_extrema=True (clip-sharded generation under a process group): the extrema are MAX-reduced over all ranks
        first, so every rank centres with the whole batch's pair and the shards equal a single-process run of the
        unsharded batch bit for bit; the default centres per shard (no data-path collective)."""
        if allow_grad:
            need_graph = torch.is_grad_enabled() and dec.requires_grad
            wavs = (_VocodeWithGrad.apply(dec, self) if need_graph else self.vocode(dec)).float()
            return wavs - (wavs.max() + wavs.min()) / 2
        wav = self.vocode(dec)
        scratch = torch.empty(4, dtype=torch.float32, device=wav.device)
        centred = torch.empty_like(wav) if return_float else None
        pcm = None if return_float else torch.empty(wav.shape, dtype=torch.int16, device=wav.device)
        with torch.cuda.device(self.device):
            if world_extrema:
                from . import dist_util
                mm = torch.empty(2, dtype=torch.float32, device=wav.device)
                N.check(N.lib().ctta_wav_extrema(N.ptr(wav), wav.numel(), N.ptr(scratch), N.ptr(mm), N.stream_ptr()))
                dist_util.global_wav_extrema_(mm)
                N.check(N.lib().ctta_wav_center(N.ptr(wav), wav.numel(), N.ptr(mm), N.ptr(scratch), N.ptr(centred), N.ptr(pcm),
                                                N.stream_ptr()))
            else:
                N.check(N.lib().ctta_wav_finalize(N.ptr(wav), wav.numel(), N.ptr(scratch), N.ptr(centred), N.ptr(pcm),
                                                  N.stream_ptr()))
        return centred if return_float else pcm.cpu().numpy()

    def _read_taps(self, which):
        if which == "vae":
            return N.read_taps("ctta_vae", self._h_vae, self.device)
        return N.read_taps("ctta_hifigan", self._h_voc, self.device)
