"""The host side of the sign planes (no GPU): the route question nimg_conv2d_pool_sign_ok answers from the dispatch's own predicate,
and the reference packing the GPU tests compare with (tests/fan_signs_cases.py)."""
import numpy as np

import fan_signs_cases as S
from neural_imaging_amd import _lib

IN, OUT = 1, 2          # include/nimg.h NIMG_BF16_IN, NIMG_BF16_OUT


def test_only_the_ring_routes_write_a_plane():
    ok = _lib.load().nimg_conv2d_pool_sign_ok
    # (cin, cout, n, h, wd, ks, flags): 384 workgroups of 64 channels and a ring shape
    assert ok(32, 128, 48, 32, 32, 5, IN | OUT) == 1 and ok(32, 64, 96, 32, 32, 5, IN | OUT) == 1
    assert ok(32, 64, 320, 128, 128, 5, IN | OUT) == 1 and ok(64, 128, 320, 64, 64, 5, IN | OUT) == 1      # the FAN's conv2 / conv3 at 320 images
    assert ok(32, 128, 47, 32, 32, 5, IN | OUT) == 0 and ok(32, 64, 95, 32, 32, 5, IN | OUT) == 0          # 32-channel tile below 384
    assert ok(32, 64, 1536, 16, 16, 5, IN | OUT) == 0                     # the 64-channel ring needs 32 rows
    assert ok(32, 128, 192, 16, 16, 5, IN | OUT) == 1                     # the 128-channel one does not
    assert ok(32, 128, 48, 32, 32, 3, IN | OUT) == 0                      # 3x3
    assert ok(32, 128, 48, 32, 32, 5, IN) == 0 and ok(32, 128, 48, 32, 32, 5, OUT) == 0      # float32 storage on either side
    assert ok(24, 128, 48, 32, 32, 5, IN | OUT) == 0 and ok(32, 96, 96, 32, 32, 5, IN | OUT) == 0      # whole 16-channel chunks in, 64 out
    assert ok(32, 128, 48, 31, 32, 5, IN | OUT) == 0 and ok(32, 128, 0, 32, 32, 5, IN | OUT) == 0


def test_reference_packing():
    vals = np.array([[0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45,      # 1e-45 rounds to +0 in bf16
                      2.0, 3.0, -2.0, 0.5, 1e-38, -1e-38, 9.2e-41, 4.5e-41]], np.float32).reshape(1, 1, 1, 16)
    bits = S.bf16_bits(vals)
    plane = S.pack_signs(bits)
    assert plane.shape == (1, 1, 1, 2) and plane.dtype == np.uint8
    assert plane[0, 0, 0, 0] == 0b00010100 and plane[0, 0, 0, 1] == 0b01011011
    special = S.pack_signs(S.SPECIAL_BF16[:8].view(np.int16).reshape(1, 1, 1, 8))      # +0 -0 +den -den +inf -inf +nan -nan
    assert special[0, 0, 0, 0] == 0b00010100
    o = S.consumer_operands(S.CONSUMER_SHAPES[2], 'full')
    u = o['act_bits'].view(np.uint16)
    assert all((u == p).any() for p in S.SPECIAL_BF16) and o['act_bits'].shape == (2, 32, 32, 32)
