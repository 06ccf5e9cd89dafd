"""The LoRA parity cases: configs and deterministic adapter values, shared by make_golden_lora.py (reference side) and the
LoRA tests, so that `lora_gdm_tiny.npz` only needs to hold the reference's OUTPUTS.

`cases.TINY_UNET` cannot carry the reference's adapters: its file name says "light", so setup_lora sizes them to
`C * 255 // 256` (80 -> 79), which is not the attention's inner width 3 * 26 = 78, and the reference raises a shape error.
The light-style case below has 40 -> 39 = 3 * 13 and 64 -> 63 = 3 * 21 = 7 * 9; the full-style case has inner width =
channel count at every level (8 / 16 / 8 lanes per head)."""
import numpy as np

import cases
from consistencytta_amd import spec

LORA_TINY_LIGHT = dict(cases.TINY_UNET, block_out_channels=[40, 64, 64, 64], attention_head_dim=[3, 3, 7, 7])
LORA_TINY_FULL = dict(cases.TINY_UNET, block_out_channels=[40, 80, 80, 80], attention_head_dim=[5, 5, 10, 10])
RANK = 4
DOWN_STD, UP_STD = 0.25, 0.08      # down as LoRALinearLayer's init (std 1 / rank); up non-zero so the adapters matter
B, H, W, L = 3, 32, 8, 6           # the sizes of gdm_tiny


def lora_weights(cfg, seed=0, up_std=UP_STD):
    """name -> fp32 tensor for every adapter tensor of `cfg` (uniform values of the stated standard deviation)"""
    out = {}
    for k, shape in spec.lora_param_spec(cfg, RANK).items():
        std = DOWN_STD if k.endswith("down.weight") else up_std
        out[k] = cases.t(spec.det_uniform("lora." + k, shape, seed) * np.float32(std * np.sqrt(3.0)))
    return out
