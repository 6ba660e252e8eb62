"""Handle creation over the whole request matrix: every entry point x distribution word (each flag bit alone) x dtype x three net shapes, one table.

CPU: every row is refused with its own reason, or gets as far as "no HIP device" -- the refusals stand in front of the first HIP call.
GPU: every accepted row creates its handle, runs one step and one train step of 33 rows (a full 16- / 32-row block and a ragged one) and must have
enqueued exactly the kernels of its row; then ppo_dist_init, with the collective library made unloadable, must either refuse the handle for the flag
of its row (the flag took effect -- or, on a categorical handle's PPO_ACT_SHAPE_KERNELS, was asked for) or get as far as loading the library.

The table pins what the scattered per-feature tests do not: the flags that are accepted and change nothing, and asked against took effect for every
head on a shape that does not qualify.  Its last column was recorded from the library of the commit before create_handle was split into stages
(built outside the package, PPO_HIP_LIBRARY); the GPU test prints what it found for every row, and a row changes only with the behaviour it states."""
import ctypes as C

import numpy as np
import pytest

F32, BF16 = 0, 1
NVEC = (3, 5, 2, 8)
# (obs, act, hidden): the narrow family's static shape (tests/test_narrow_multi_discrete.py) | the [256,256] pair's (tests/test_pair_multi_binary.py) |
# neither (tests/test_pair_multi_binary.py's fallback)
SHAPES = {"narrow": (18, 18, (64, 64)), "pair": (18, 18, (256, 256)), "neither": (18, 18, (256, 256, 256))}
NO_DEVICE = "ppo_create: no HIP device available"
FLAG_NAMES = ("PPO_ACT_SHAPE_KERNELS", "PPO_ACT_BF16_HEAD", "PPO_ACT_PAIR_KERNELS", "PPO_ACT_BF16_MULTI_HEAD", "PPO_ACT_BINARY_SHAPE_KERNELS", "PPO_ACT_BINARY_PAIR_KERNELS")

# (entry point, action_dist word of ppo_create_ex / flags word of ppo_create_multi_ex, nvec, compute_dtype, shape,
#  the refusal | (the kernels enqueued, the flag ppo_dist_init refuses the handle for or ""))
TABLE = [
    ("ppo_create_ex", 0x0, None, F32, "narrow", ('narrow_step_kernel<static> narrow_train_kernel<static>', '')),
    ("ppo_create_ex", 0x100, None, F32, "narrow", ('narrow_step_kernel<static> narrow_train_kernel<static>', '')),
    ("ppo_create_ex", 0x200, None, F32, "narrow", ('narrow_step_kernel<static> narrow_train_kernel<static>', '')),
    ("ppo_create_ex", 0x400, None, F32, "narrow", ('narrow_step_kernel<static> narrow_train_kernel<static>', '')),
    ("ppo_create_ex", 0x1000, None, F32, "narrow", 'ppo_create_ex: unknown action_dist 4096'),
    ("ppo_create_ex", 0x2000, None, F32, "narrow", 'ppo_create_ex: unknown action_dist 8192'),
    ("ppo_create_ex", 0x4000, None, F32, "narrow", 'ppo_create_ex: unknown action_dist 16384'),
    ("ppo_create_ex", 0x1, None, F32, "narrow", ('grad_reduce_kernel policy_step_kernel<cat> train_fwd_bwd_kernel<cat> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x101, None, F32, "narrow", ('narrow_step_kernel<cat> narrow_train_kernel<cat>', 'PPO_ACT_SHAPE_KERNELS')),
    ("ppo_create_ex", 0x201, None, F32, "narrow", ('grad_reduce_kernel policy_step_kernel<cat> train_fwd_bwd_kernel<cat> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x401, None, F32, "narrow", ('grad_reduce_kernel policy_step_kernel<cat> train_fwd_bwd_kernel<cat> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x1001, None, F32, "narrow", 'ppo_create_ex: unknown action_dist 4097'),
    ("ppo_create_ex", 0x2001, None, F32, "narrow", 'ppo_create_ex: unknown action_dist 8193'),
    ("ppo_create_ex", 0x4001, None, F32, "narrow", 'ppo_create_ex: unknown action_dist 16385'),
    ("ppo_create_ex", 0x2, None, F32, "narrow", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x102, None, F32, "narrow", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x202, None, F32, "narrow", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x402, None, F32, "narrow", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x1002, None, F32, "narrow", 'ppo_create_ex: unknown action_dist 4098'),
    ("ppo_create_ex", 0x2002, None, F32, "narrow", 'ppo_create_ex: unknown action_dist 8194'),
    ("ppo_create_ex", 0x4002, None, F32, "narrow", 'ppo_create_ex: unknown action_dist 16386'),
    ("ppo_create_ex", 0x3, None, F32, "narrow", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x103, None, F32, "narrow", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x203, None, F32, "narrow", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x403, None, F32, "narrow", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x1003, None, F32, "narrow", 'ppo_create_ex: unknown action_dist 4099'),
    ("ppo_create_ex", 0x2003, None, F32, "narrow", ('narrow_step_kernel<mbin> narrow_train_kernel<mbin>', 'PPO_ACT_BINARY_SHAPE_KERNELS')),
    ("ppo_create_ex", 0x4003, None, F32, "narrow", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x0, None, BF16, "narrow", ('bf16_reduce_adam_kernel bf16_step_sequence bf16_train_sequence', '')),
    ("ppo_create_ex", 0x100, None, BF16, "narrow", ('bf16_reduce_adam_kernel bf16_step_sequence bf16_train_sequence', '')),
    ("ppo_create_ex", 0x200, None, BF16, "narrow", ('bf16_reduce_adam_kernel bf16_step_sequence bf16_train_sequence', '')),
    ("ppo_create_ex", 0x400, None, BF16, "narrow", ('bf16_reduce_adam_kernel bf16_step_sequence bf16_train_sequence', '')),
    ("ppo_create_ex", 0x1000, None, BF16, "narrow", 'ppo_create_ex: unknown action_dist 4096'),
    ("ppo_create_ex", 0x2000, None, BF16, "narrow", 'ppo_create_ex: unknown action_dist 8192'),
    ("ppo_create_ex", 0x4000, None, BF16, "narrow", 'ppo_create_ex: unknown action_dist 16384'),
    ("ppo_create_ex", 0x1, None, BF16, "narrow", 'ppo_create_ex: PPO_ACT_CATEGORICAL with compute_dtype PPO_BF16 is not supported without PPO_ACT_BF16_HEAD'),
    ("ppo_create_ex", 0x101, None, BF16, "narrow", 'ppo_create_ex: PPO_ACT_CATEGORICAL with compute_dtype PPO_BF16 is not supported without PPO_ACT_BF16_HEAD'),
    ("ppo_create_ex", 0x201, None, BF16, "narrow", ('bf16_reduce_adam_kernel bf16_step_sequence<cat> bf16_train_sequence<cat>', 'PPO_ACT_BF16_HEAD')),
    ("ppo_create_ex", 0x401, None, BF16, "narrow", 'ppo_create_ex: PPO_ACT_CATEGORICAL with compute_dtype PPO_BF16 is not supported without PPO_ACT_BF16_HEAD'),
    ("ppo_create_ex", 0x1001, None, BF16, "narrow", 'ppo_create_ex: unknown action_dist 4097'),
    ("ppo_create_ex", 0x2001, None, BF16, "narrow", 'ppo_create_ex: unknown action_dist 8193'),
    ("ppo_create_ex", 0x4001, None, BF16, "narrow", 'ppo_create_ex: unknown action_dist 16385'),
    ("ppo_create_ex", 0x2, None, BF16, "narrow", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x102, None, BF16, "narrow", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x202, None, BF16, "narrow", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x402, None, BF16, "narrow", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x1002, None, BF16, "narrow", 'ppo_create_ex: unknown action_dist 4098'),
    ("ppo_create_ex", 0x2002, None, BF16, "narrow", 'ppo_create_ex: unknown action_dist 8194'),
    ("ppo_create_ex", 0x4002, None, BF16, "narrow", 'ppo_create_ex: unknown action_dist 16386'),
    ("ppo_create_ex", 0x3, None, BF16, "narrow", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x103, None, BF16, "narrow", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x203, None, BF16, "narrow", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x403, None, BF16, "narrow", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x1003, None, BF16, "narrow", 'ppo_create_ex: unknown action_dist 4099'),
    ("ppo_create_ex", 0x2003, None, BF16, "narrow", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x4003, None, BF16, "narrow", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x0, NVEC, F32, "narrow", ('grad_reduce_kernel policy_step_kernel<mcat> train_fwd_bwd_kernel<mcat> weight_grad_kernel', '')),
    ("ppo_create_multi_ex", 0x100, NVEC, F32, "narrow", ('narrow_step_kernel<mcat> narrow_train_kernel<mcat>', 'PPO_ACT_SHAPE_KERNELS')),
    ("ppo_create_multi_ex", 0x200, NVEC, F32, "narrow", ('grad_reduce_kernel policy_step_kernel<mcat> train_fwd_bwd_kernel<mcat> weight_grad_kernel', '')),
    ("ppo_create_multi_ex", 0x400, NVEC, F32, "narrow", ('grad_reduce_kernel policy_step_kernel<mcat> train_fwd_bwd_kernel<mcat> weight_grad_kernel', '')),
    ("ppo_create_multi_ex", 0x800, NVEC, F32, "narrow", 'ppo_create_multi_ex: unknown flag bit 0x800'),
    ("ppo_create_multi_ex", 0x1000, NVEC, F32, "narrow", ('grad_reduce_kernel policy_step_kernel<mcat> train_fwd_bwd_kernel<mcat> weight_grad_kernel', '')),
    ("ppo_create_multi_ex", 0x2000, NVEC, F32, "narrow", 'ppo_create_multi_ex: unknown flag bit 0x2000'),
    ("ppo_create_multi_ex", 0x4000, NVEC, F32, "narrow", 'ppo_create_multi_ex: unknown flag bit 0x4000'),
    ("ppo_create_multi_ex", 0x0, NVEC, BF16, "narrow", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x100, NVEC, BF16, "narrow", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x200, NVEC, BF16, "narrow", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x400, NVEC, BF16, "narrow", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x800, NVEC, BF16, "narrow", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x1000, NVEC, BF16, "narrow", ('bf16_reduce_adam_kernel bf16_step_sequence<mcat> bf16_train_sequence<mcat>', 'PPO_ACT_BF16_MULTI_HEAD')),
    ("ppo_create_multi_ex", 0x2000, NVEC, BF16, "narrow", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x4000, NVEC, BF16, "narrow", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x0, None, F32, "pair", ('policy_step_kernel train8_kernel weight_grad_assemble_kernel', '')),
    ("ppo_create_ex", 0x100, None, F32, "pair", ('policy_step_kernel train8_kernel weight_grad_assemble_kernel', '')),
    ("ppo_create_ex", 0x200, None, F32, "pair", ('policy_step_kernel train8_kernel weight_grad_assemble_kernel', '')),
    ("ppo_create_ex", 0x400, None, F32, "pair", ('policy_step_kernel train8_kernel weight_grad_assemble_kernel', '')),
    ("ppo_create_ex", 0x1000, None, F32, "pair", 'ppo_create_ex: unknown action_dist 4096'),
    ("ppo_create_ex", 0x2000, None, F32, "pair", 'ppo_create_ex: unknown action_dist 8192'),
    ("ppo_create_ex", 0x4000, None, F32, "pair", 'ppo_create_ex: unknown action_dist 16384'),
    ("ppo_create_ex", 0x1, None, F32, "pair", ('grad_reduce_kernel policy_step_kernel<cat> train_fwd_bwd_kernel<cat> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x101, None, F32, "pair", ('grad_reduce_kernel policy_step_kernel<cat> train_fwd_bwd_kernel<cat> weight_grad_kernel', 'PPO_ACT_SHAPE_KERNELS')),
    ("ppo_create_ex", 0x201, None, F32, "pair", ('grad_reduce_kernel policy_step_kernel<cat> train_fwd_bwd_kernel<cat> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x401, None, F32, "pair", ('policy_step_kernel<cat> train8_kernel<cat> weight_grad_assemble_kernel', 'PPO_ACT_PAIR_KERNELS')),
    ("ppo_create_ex", 0x1001, None, F32, "pair", 'ppo_create_ex: unknown action_dist 4097'),
    ("ppo_create_ex", 0x2001, None, F32, "pair", 'ppo_create_ex: unknown action_dist 8193'),
    ("ppo_create_ex", 0x4001, None, F32, "pair", 'ppo_create_ex: unknown action_dist 16385'),
    ("ppo_create_ex", 0x2, None, F32, "pair", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x102, None, F32, "pair", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x202, None, F32, "pair", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x402, None, F32, "pair", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x1002, None, F32, "pair", 'ppo_create_ex: unknown action_dist 4098'),
    ("ppo_create_ex", 0x2002, None, F32, "pair", 'ppo_create_ex: unknown action_dist 8194'),
    ("ppo_create_ex", 0x4002, None, F32, "pair", 'ppo_create_ex: unknown action_dist 16386'),
    ("ppo_create_ex", 0x3, None, F32, "pair", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x103, None, F32, "pair", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x203, None, F32, "pair", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x403, None, F32, "pair", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x1003, None, F32, "pair", 'ppo_create_ex: unknown action_dist 4099'),
    ("ppo_create_ex", 0x2003, None, F32, "pair", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x4003, None, F32, "pair", ('policy_step_kernel<mbin> weight_grad_assemble_kernel', 'PPO_ACT_BINARY_PAIR_KERNELS')),
    ("ppo_create_ex", 0x0, None, BF16, "pair", ('bf16_reduce_adam_kernel bf16_step_sequence bf16_train_sequence', '')),
    ("ppo_create_ex", 0x100, None, BF16, "pair", ('bf16_reduce_adam_kernel bf16_step_sequence bf16_train_sequence', '')),
    ("ppo_create_ex", 0x200, None, BF16, "pair", ('bf16_reduce_adam_kernel bf16_step_sequence bf16_train_sequence', '')),
    ("ppo_create_ex", 0x400, None, BF16, "pair", ('bf16_reduce_adam_kernel bf16_step_sequence bf16_train_sequence', '')),
    ("ppo_create_ex", 0x1000, None, BF16, "pair", 'ppo_create_ex: unknown action_dist 4096'),
    ("ppo_create_ex", 0x2000, None, BF16, "pair", 'ppo_create_ex: unknown action_dist 8192'),
    ("ppo_create_ex", 0x4000, None, BF16, "pair", 'ppo_create_ex: unknown action_dist 16384'),
    ("ppo_create_ex", 0x1, None, BF16, "pair", 'ppo_create_ex: PPO_ACT_CATEGORICAL with compute_dtype PPO_BF16 is not supported without PPO_ACT_BF16_HEAD'),
    ("ppo_create_ex", 0x101, None, BF16, "pair", 'ppo_create_ex: PPO_ACT_CATEGORICAL with compute_dtype PPO_BF16 is not supported without PPO_ACT_BF16_HEAD'),
    ("ppo_create_ex", 0x201, None, BF16, "pair", ('bf16_reduce_adam_kernel bf16_step_sequence<cat> bf16_train_sequence<cat>', 'PPO_ACT_BF16_HEAD')),
    ("ppo_create_ex", 0x401, None, BF16, "pair", 'ppo_create_ex: PPO_ACT_CATEGORICAL with compute_dtype PPO_BF16 is not supported without PPO_ACT_BF16_HEAD'),
    ("ppo_create_ex", 0x1001, None, BF16, "pair", 'ppo_create_ex: unknown action_dist 4097'),
    ("ppo_create_ex", 0x2001, None, BF16, "pair", 'ppo_create_ex: unknown action_dist 8193'),
    ("ppo_create_ex", 0x4001, None, BF16, "pair", 'ppo_create_ex: unknown action_dist 16385'),
    ("ppo_create_ex", 0x2, None, BF16, "pair", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x102, None, BF16, "pair", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x202, None, BF16, "pair", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x402, None, BF16, "pair", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x1002, None, BF16, "pair", 'ppo_create_ex: unknown action_dist 4098'),
    ("ppo_create_ex", 0x2002, None, BF16, "pair", 'ppo_create_ex: unknown action_dist 8194'),
    ("ppo_create_ex", 0x4002, None, BF16, "pair", 'ppo_create_ex: unknown action_dist 16386'),
    ("ppo_create_ex", 0x3, None, BF16, "pair", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x103, None, BF16, "pair", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x203, None, BF16, "pair", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x403, None, BF16, "pair", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x1003, None, BF16, "pair", 'ppo_create_ex: unknown action_dist 4099'),
    ("ppo_create_ex", 0x2003, None, BF16, "pair", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x4003, None, BF16, "pair", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x0, NVEC, F32, "pair", ('grad_reduce_kernel policy_step_kernel<mcat> train_fwd_bwd_kernel<mcat> weight_grad_kernel', '')),
    ("ppo_create_multi_ex", 0x100, NVEC, F32, "pair", ('grad_reduce_kernel policy_step_kernel<mcat> train_fwd_bwd_kernel<mcat> weight_grad_kernel', '')),
    ("ppo_create_multi_ex", 0x200, NVEC, F32, "pair", ('grad_reduce_kernel policy_step_kernel<mcat> train_fwd_bwd_kernel<mcat> weight_grad_kernel', '')),
    ("ppo_create_multi_ex", 0x400, NVEC, F32, "pair", ('policy_step_kernel<mcat> train8_kernel<mcat> weight_grad_assemble_kernel', 'PPO_ACT_PAIR_KERNELS')),
    ("ppo_create_multi_ex", 0x800, NVEC, F32, "pair", 'ppo_create_multi_ex: unknown flag bit 0x800'),
    ("ppo_create_multi_ex", 0x1000, NVEC, F32, "pair", ('grad_reduce_kernel policy_step_kernel<mcat> train_fwd_bwd_kernel<mcat> weight_grad_kernel', '')),
    ("ppo_create_multi_ex", 0x2000, NVEC, F32, "pair", 'ppo_create_multi_ex: unknown flag bit 0x2000'),
    ("ppo_create_multi_ex", 0x4000, NVEC, F32, "pair", 'ppo_create_multi_ex: unknown flag bit 0x4000'),
    ("ppo_create_multi_ex", 0x0, NVEC, BF16, "pair", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x100, NVEC, BF16, "pair", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x200, NVEC, BF16, "pair", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x400, NVEC, BF16, "pair", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x800, NVEC, BF16, "pair", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x1000, NVEC, BF16, "pair", ('bf16_reduce_adam_kernel bf16_step_sequence<mcat> bf16_train_sequence<mcat>', 'PPO_ACT_BF16_MULTI_HEAD')),
    ("ppo_create_multi_ex", 0x2000, NVEC, BF16, "pair", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x4000, NVEC, BF16, "pair", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x0, None, F32, "neither", ('grad_reduce_kernel policy_step_kernel train_fwd_bwd_kernel weight_grad_kernel', '')),
    ("ppo_create_ex", 0x100, None, F32, "neither", ('grad_reduce_kernel policy_step_kernel train_fwd_bwd_kernel weight_grad_kernel', '')),
    ("ppo_create_ex", 0x200, None, F32, "neither", ('grad_reduce_kernel policy_step_kernel train_fwd_bwd_kernel weight_grad_kernel', '')),
    ("ppo_create_ex", 0x400, None, F32, "neither", ('grad_reduce_kernel policy_step_kernel train_fwd_bwd_kernel weight_grad_kernel', '')),
    ("ppo_create_ex", 0x1000, None, F32, "neither", 'ppo_create_ex: unknown action_dist 4096'),
    ("ppo_create_ex", 0x2000, None, F32, "neither", 'ppo_create_ex: unknown action_dist 8192'),
    ("ppo_create_ex", 0x4000, None, F32, "neither", 'ppo_create_ex: unknown action_dist 16384'),
    ("ppo_create_ex", 0x1, None, F32, "neither", ('grad_reduce_kernel policy_step_kernel<cat> train_fwd_bwd_kernel<cat> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x101, None, F32, "neither", ('grad_reduce_kernel policy_step_kernel<cat> train_fwd_bwd_kernel<cat> weight_grad_kernel', 'PPO_ACT_SHAPE_KERNELS')),
    ("ppo_create_ex", 0x201, None, F32, "neither", ('grad_reduce_kernel policy_step_kernel<cat> train_fwd_bwd_kernel<cat> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x401, None, F32, "neither", ('grad_reduce_kernel policy_step_kernel<cat> train_fwd_bwd_kernel<cat> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x1001, None, F32, "neither", 'ppo_create_ex: unknown action_dist 4097'),
    ("ppo_create_ex", 0x2001, None, F32, "neither", 'ppo_create_ex: unknown action_dist 8193'),
    ("ppo_create_ex", 0x4001, None, F32, "neither", 'ppo_create_ex: unknown action_dist 16385'),
    ("ppo_create_ex", 0x2, None, F32, "neither", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x102, None, F32, "neither", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x202, None, F32, "neither", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x402, None, F32, "neither", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x1002, None, F32, "neither", 'ppo_create_ex: unknown action_dist 4098'),
    ("ppo_create_ex", 0x2002, None, F32, "neither", 'ppo_create_ex: unknown action_dist 8194'),
    ("ppo_create_ex", 0x4002, None, F32, "neither", 'ppo_create_ex: unknown action_dist 16386'),
    ("ppo_create_ex", 0x3, None, F32, "neither", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x103, None, F32, "neither", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x203, None, F32, "neither", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x403, None, F32, "neither", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x1003, None, F32, "neither", 'ppo_create_ex: unknown action_dist 4099'),
    ("ppo_create_ex", 0x2003, None, F32, "neither", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x4003, None, F32, "neither", ('grad_reduce_kernel policy_step_kernel<mbin> train_fwd_bwd_kernel<mbin> weight_grad_kernel', '')),
    ("ppo_create_ex", 0x0, None, BF16, "neither", ('bf16_reduce_adam_kernel bf16_step_sequence bf16_train_sequence', '')),
    ("ppo_create_ex", 0x100, None, BF16, "neither", ('bf16_reduce_adam_kernel bf16_step_sequence bf16_train_sequence', '')),
    ("ppo_create_ex", 0x200, None, BF16, "neither", ('bf16_reduce_adam_kernel bf16_step_sequence bf16_train_sequence', '')),
    ("ppo_create_ex", 0x400, None, BF16, "neither", ('bf16_reduce_adam_kernel bf16_step_sequence bf16_train_sequence', '')),
    ("ppo_create_ex", 0x1000, None, BF16, "neither", 'ppo_create_ex: unknown action_dist 4096'),
    ("ppo_create_ex", 0x2000, None, BF16, "neither", 'ppo_create_ex: unknown action_dist 8192'),
    ("ppo_create_ex", 0x4000, None, BF16, "neither", 'ppo_create_ex: unknown action_dist 16384'),
    ("ppo_create_ex", 0x1, None, BF16, "neither", 'ppo_create_ex: PPO_ACT_CATEGORICAL with compute_dtype PPO_BF16 is not supported without PPO_ACT_BF16_HEAD'),
    ("ppo_create_ex", 0x101, None, BF16, "neither", 'ppo_create_ex: PPO_ACT_CATEGORICAL with compute_dtype PPO_BF16 is not supported without PPO_ACT_BF16_HEAD'),
    ("ppo_create_ex", 0x201, None, BF16, "neither", ('bf16_reduce_adam_kernel bf16_step_sequence<cat> bf16_train_sequence<cat>', 'PPO_ACT_BF16_HEAD')),
    ("ppo_create_ex", 0x401, None, BF16, "neither", 'ppo_create_ex: PPO_ACT_CATEGORICAL with compute_dtype PPO_BF16 is not supported without PPO_ACT_BF16_HEAD'),
    ("ppo_create_ex", 0x1001, None, BF16, "neither", 'ppo_create_ex: unknown action_dist 4097'),
    ("ppo_create_ex", 0x2001, None, BF16, "neither", 'ppo_create_ex: unknown action_dist 8193'),
    ("ppo_create_ex", 0x4001, None, BF16, "neither", 'ppo_create_ex: unknown action_dist 16385'),
    ("ppo_create_ex", 0x2, None, BF16, "neither", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x102, None, BF16, "neither", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x202, None, BF16, "neither", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x402, None, BF16, "neither", 'ppo_create_ex: unknown action_dist 2'),
    ("ppo_create_ex", 0x1002, None, BF16, "neither", 'ppo_create_ex: unknown action_dist 4098'),
    ("ppo_create_ex", 0x2002, None, BF16, "neither", 'ppo_create_ex: unknown action_dist 8194'),
    ("ppo_create_ex", 0x4002, None, BF16, "neither", 'ppo_create_ex: unknown action_dist 16386'),
    ("ppo_create_ex", 0x3, None, BF16, "neither", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x103, None, BF16, "neither", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x203, None, BF16, "neither", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x403, None, BF16, "neither", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x1003, None, BF16, "neither", 'ppo_create_ex: unknown action_dist 4099'),
    ("ppo_create_ex", 0x2003, None, BF16, "neither", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_ex", 0x4003, None, BF16, "neither", 'ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x0, NVEC, F32, "neither", ('grad_reduce_kernel policy_step_kernel<mcat> train_fwd_bwd_kernel<mcat> weight_grad_kernel', '')),
    ("ppo_create_multi_ex", 0x100, NVEC, F32, "neither", ('grad_reduce_kernel policy_step_kernel<mcat> train_fwd_bwd_kernel<mcat> weight_grad_kernel', '')),
    ("ppo_create_multi_ex", 0x200, NVEC, F32, "neither", ('grad_reduce_kernel policy_step_kernel<mcat> train_fwd_bwd_kernel<mcat> weight_grad_kernel', '')),
    ("ppo_create_multi_ex", 0x400, NVEC, F32, "neither", ('grad_reduce_kernel policy_step_kernel<mcat> train_fwd_bwd_kernel<mcat> weight_grad_kernel', '')),
    ("ppo_create_multi_ex", 0x800, NVEC, F32, "neither", 'ppo_create_multi_ex: unknown flag bit 0x800'),
    ("ppo_create_multi_ex", 0x1000, NVEC, F32, "neither", ('grad_reduce_kernel policy_step_kernel<mcat> train_fwd_bwd_kernel<mcat> weight_grad_kernel', '')),
    ("ppo_create_multi_ex", 0x2000, NVEC, F32, "neither", 'ppo_create_multi_ex: unknown flag bit 0x2000'),
    ("ppo_create_multi_ex", 0x4000, NVEC, F32, "neither", 'ppo_create_multi_ex: unknown flag bit 0x4000'),
    ("ppo_create_multi_ex", 0x0, NVEC, BF16, "neither", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x100, NVEC, BF16, "neither", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x200, NVEC, BF16, "neither", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x400, NVEC, BF16, "neither", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x800, NVEC, BF16, "neither", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x1000, NVEC, BF16, "neither", ('bf16_reduce_adam_kernel bf16_step_sequence<mcat> bf16_train_sequence<mcat>', 'PPO_ACT_BF16_MULTI_HEAD')),
    ("ppo_create_multi_ex", 0x2000, NVEC, BF16, "neither", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
    ("ppo_create_multi_ex", 0x4000, NVEC, BF16, "neither", 'ppo_create_multi: compute_dtype PPO_BF16 is not supported'),
]


def create(entry, word, nvec, dtype, shape):
    """-> (rc, handle, the create error)"""
    from ppo_cpp_amd import capi
    lib = capi.load_library()
    O, A, hidden = SHAPES[shape]
    cfg = capi.PPOConfig()
    lib.ppo_config_default(C.byref(cfg), O, A, len(hidden), (C.c_int32 * len(hidden))(*hidden))
    cfg.compute_dtype = dtype
    h = C.c_void_p()
    if entry == "ppo_create_ex":
        rc = lib.ppo_create_ex(C.byref(cfg), word, C.byref(h))
    else:
        assert entry == "ppo_create_multi_ex"
        rc = lib.ppo_create_multi_ex(C.byref(cfg), (C.c_int32 * len(nvec))(*nvec), len(nvec), word, C.byref(h))
    return rc, h, lib.ppo_last_error(None).decode()


def wrap(h, shape):
    """the handle under the Python layer's methods (PPOHip's constructor takes keywords, not the words of this table)"""
    from ppo_cpp_amd import capi
    g = capi.PPOHip.__new__(capi.PPOHip)
    g.lib, g.h = capi.load_library(), h
    g.O, g.A, _ = SHAPES[shape]
    dist = g.lib.ppo_action_dist(h)
    g.action_dist = {v: k for k, v in capi.ACTION_DISTS.items()}[dist]
    g._act_shape = (g.A,) if dist in (0, 3) else (len(NVEC),) if dist == 2 else ()
    return g


def observe(g):
    """-> (the kernels one step and one train step of 33 rows enqueued, the flag ppo_dist_init refuses the handle for or "")"""
    from ppo_cpp_amd import capi
    rng = np.random.RandomState(0)
    n = 33
    obs = rng.normal(size=(n, g.O)).astype(np.float32)
    act, v, nlp = g.step(obs)
    adv = rng.normal(size=n).astype(np.float32)
    g.train_step(3e-4, 0.2, obs, act, adv, v + adv, nlp, v)
    names = " ".join(sorted(k for k, c in g.kernel_counts(all_rows=True).items() if c))
    try:
        g.dist_init(1, 0, bytes(128))
        raise AssertionError("ppo_dist_init went through without a collective library")
    except capi.PPOHipError as e:
        msg = str(e)
    if "PPO_RCCL_LIBRARY: cannot load" in msg:
        return names, ""
    assert msg.startswith("ppo_dist_init: data parallel is not supported for a ") and "created with " in msg, msg
    flag = msg.split("created with ")[1].split()[0]
    assert flag in FLAG_NAMES, msg
    return names, flag


def test_table_covers_the_matrix():
    ex = [0, 0x100, 0x200, 0x400, 0x1000, 0x2000, 0x4000]
    want = {("ppo_create_ex", d | f, None, t, s) for d in (0, 1, 2, 3) for f in ex for t in (F32, BF16) for s in SHAPES}
    want |= {("ppo_create_multi_ex", f, NVEC, t, s) for f in ex + [0x800] for t in (F32, BF16) for s in SHAPES}
    assert {r[:5] for r in TABLE} == want and len(TABLE) == len(want) == 216


def test_refusals_stand_in_front_of_the_first_hip_call():
    """needs a machine WITHOUT a GPU to say anything about the accepted rows: there they end in "no HIP device"; with one, those rows create a handle (and close it)"""
    from ppo_cpp_amd import capi
    lib = capi.load_library()
    for entry, word, nvec, dtype, shape, expect in TABLE:
        rc, h, err = create(entry, word, nvec, dtype, shape)
        row = (entry, hex(word), dtype, shape, err)
        if isinstance(expect, str):
            assert rc != 0 and expect in err, row
        elif rc == 0:
            lib.ppo_destroy(h)
        else:
            assert NO_DEVICE in err, row


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernels_and_data_parallel_outcome_of_every_accepted_row(shape, monkeypatch):
    monkeypatch.setenv("PPO_RCCL_LIBRARY", "/nonexistent/no_collective_library.so")       # ppo_dist_init gets as far as loading it, no further
    found = []
    for entry, word, nvec, dtype, s, expect in TABLE:
        if s != shape or isinstance(expect, str):
            continue
        rc, h, err = create(entry, word, nvec, dtype, shape)
        assert rc == 0, (entry, hex(word), dtype, shape, err)
        g = wrap(h, shape)
        got = observe(g)
        g.close()
        print(entry, hex(word), dtype, shape, got)
        if got != expect:
            found.append((entry, hex(word), dtype, shape, got, expect))
    assert not found, found
