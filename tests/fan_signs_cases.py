"""Operands and the reference packing of tests/test_gpu_fan_signs.py, shared with its child process (tests/fan_signs_child.py).

A sign plane is (N, H, W, C / 8) uint8 next to a bf16 tensor (N, H, W, C): bit e of byte c / 8 is 1 iff the STORED bf16 value of
channel c + e is > 0 - so +0, -0, NaN and every negative value give 0 (include/nimg.h)."""
import numpy as np
import torch

from conv_cases import full_mantissa, planted_idx
from util import ternary

# (n, h, w, cin <- cout): the input-gradient shapes of the three ring forms (conv5_ring_kernel<128 | 64 | 32, true>); with
# NIMG_TN32_BELOW=0 the first two reach their ring at this size, the third does anyway
CONSUMER_SHAPES = [(2, 32, 32, 128, 64), (2, 32, 32, 64, 128), (2, 32, 32, 32, 64)]
OPERAND_KINDS = ('ints', 'full')

# bf16 bit patterns every activation tensor of the consumer tests carries: +0, -0, the smallest denormals, +-inf, NaNs of both signs
SPECIAL_BF16 = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81], np.uint16)


def bits(t):
    """The bytes of a bf16 (or any 2-byte) device tensor as an int16 numpy array."""
    return t.contiguous().view(torch.int16).cpu().numpy()


def bf16_bits(a):
    """float32 array -> the int16 bit patterns of its bf16 (round-to-nearest-even) values."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).view(torch.int16).numpy()


def bf16_value(b):
    """int16 bf16 bit patterns -> float32 values."""
    return torch.from_numpy(np.ascontiguousarray(b, np.int16)).view(torch.bfloat16).float().numpy()


def pack_signs(act_bits):
    """The sign plane of a bf16 tensor given as int16 bit patterns (N, H, W, C), C % 8 == 0: the predicate is applied to the VALUES."""
    with np.errstate(invalid='ignore'):
        positive = bf16_value(act_bits) > 0
    return np.packbits(positive, axis=-1, bitorder='little')


def consumer_name(shape, kind):
    return '{}from{}-{}'.format(shape[3], shape[4], kind)


def consumer_operands(shape, kind):
    """Pooled gradient, arg-max bytes, weights and the masking activation (bit patterns) of one conv2d_dgrad_unpool call.  'ints':
    ternary operands (every product and sum exact); 'full': full-mantissa operands."""
    n, h, w, cin, cout = shape
    seed = 100 * cin + cout + (0 if kind == 'ints' else 7)
    if kind == 'ints':
        gp, wt = ternary((n, h // 2, w // 2, cout), seed + 1), ternary((5, 5, cin, cout), seed + 2)
    else:
        gp, wt = full_mantissa((n, h // 2, w // 2, cout), seed + 1), 0.2 * full_mantissa((5, 5, cin, cout), seed + 2)
    act = bf16_bits(full_mantissa((n, h, w, cin), seed + 3))
    flat = act.reshape(-1)
    where = np.random.default_rng(seed + 4).choice(flat.size, size=flat.size // 8, replace=False)
    flat[where] = SPECIAL_BF16.view(np.int16)[np.arange(where.size) % SPECIAL_BF16.size]
    return dict(gp=gp, w=wt.astype(np.float32), idx=planted_idx((n, h // 2, w // 2, cout), seed + 5), act_bits=act)
