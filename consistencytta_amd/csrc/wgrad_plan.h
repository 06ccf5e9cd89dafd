// Weight gradients of the engines' backward passes, host side: the PLAN of one layer (ctta_wgrad_plan, include/ctta.h) --
// route, position splits, slab geometry, scratch sizes -- worked out without touching the device (wgrad_plan.hip), and the
// two policies it is made under.  engine_backward.h launches from the plan.
#pragma once
#include "common.h"

// U-Net: launches aimed at 256 workgroups with at most 16 splits -- in a replayed distillation step one kernel has the
// device to itself 79 % of the time, so a narrower, longer launch on the side stream runs BESIDE the main stream's kernels
// and every halving of the splits halves the slab bytes (profiles/ab_r05_wgrad_splits.txt,
// profiles/gaps_distill_pipelined_r05.txt).  One-split launches add into the gradient tensors themselves; the x2-upsampling
// samplers go through im2col^T, which knows `upsample`.
constexpr ctta_wgrad_policy kWgradPolicyUnet = {256, 16, 1, 0};
// VAE decoder: one stream, so a launch should fill the device: 512 workgroups (two per CU), up to 128 splits.  At 1024 x 64
// and batch 4 a 128 -> 128 layer has four 64 x 64 tiles: 0.53 / 0.17 / 0.14 ms at 16 / 64 / 128 splits against 0.51 ms for
// the copies route; past two workgroups per CU the time rises again (profiles/vae_wgrad.txt).  The x2-upsampling
// convolutions run the same kernel over a materialised x2 copy of their input (ctta_upsample2_nearest).
constexpr ctta_wgrad_policy kWgradPolicyVae = {512, 128, 0, 1};
