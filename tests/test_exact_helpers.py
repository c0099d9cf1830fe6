"""
The exact-arithmetic helpers of tests/util.py (used by tests/test_gpu_exact.py), checked without a GPU: a float32
torch.nn.functional.conv2d on the CPU stands in for a kernel.  It must pass assert_exact against the float64 reference, and a
stand-in with one product missing, one input pixel displaced or the wrong tie rule must be rejected - the proof that the
GPU tests can fail.
"""
import numpy as np
import pytest
import torch

from oracle import tfops as T

from util import (assert_exact, assert_exact_conditions, bf16_rne, first_max_pool, lrelu_f32, small_ints, ternary, to64,
                  unpool)

SHAPES = [(2, 12, 20, 64, 48, 3), (1, 16, 16, 32, 24, 5)]


def _stand_in(x, w, b):
    """A 'kernel': float32 convolution on the CPU."""
    return T.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b)).numpy()


def test_generators_are_bf16_integers():
    t, s = ternary((4, 33, 17, 5), 1, 0.25), small_ints((4, 33, 17, 5), 2, 3)
    assert set(np.unique(t)) == {-1.0, 0.0, 1.0} and 0.2 < (t != 0).mean() < 0.3
    assert set(np.unique(s)) == {float(v) for v in range(-3, 4)}
    assert np.array_equal(bf16_rne(t), t) and np.array_equal(bf16_rne(s), s)
    assert np.array_equal(ternary((8, 8), 5), ternary((8, 8), 5)) and not np.array_equal(ternary((8, 8), 5), ternary((8, 8), 6))
    # round-to-nearest-even at the bf16 grid: 1 + 2^-8 is a tie (-> 1), 1 + 3 * 2^-8 a tie (-> 1 + 2^-6)
    assert np.array_equal(bf16_rne(np.float32([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20])),
                          [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7])


@pytest.mark.parametrize('shape', SHAPES)
def test_float32_convolution_is_exact_and_wrong_ones_are_rejected(shape):
    n, h, w, cin, cout, k = shape
    x, wt, b = small_ints((n, h, w, cin), 1), small_ints((k, k, cin, cout), 2), small_ints((cout,), 3)
    ref = T.conv2d(to64(x), to64(wt), to64(b)).numpy()
    assert_exact_conditions(T.conv2d(to64(np.abs(x)), to64(np.abs(wt)), to64(np.abs(b))).numpy(), ref, False)
    assert_exact(_stand_in(x, wt, b), ref, 'float32 stand-in')
    # one product dropped: a single non-zero weight element zeroed
    w1 = wt.copy()
    tap = tuple(np.argwhere(w1 != 0)[len(np.argwhere(w1 != 0)) // 2])
    w1[tap] = 0
    with pytest.raises(AssertionError) as e:
        assert_exact(_stand_in(x, w1, b), ref, 'dropped product')
    assert 'dropped product' in str(e.value) and 'got' in str(e.value) and 'want' in str(e.value)
    # one input pixel read from the column next to it
    x1 = x.copy()
    x1[n - 1, h // 2, w - 1] = x[n - 1, h // 2, w - 2]
    assert not np.array_equal(x1, x)
    with pytest.raises(AssertionError):
        assert_exact(_stand_in(x1, wt, b), ref, 'displaced pixel')
    # ... and the two tensors' shapes must agree
    with pytest.raises(AssertionError):
        assert_exact(ref[:, 1:], ref, 'shape')


@pytest.mark.parametrize('shape', SHAPES)
def test_arg_max_tie_rule_is_pinned(shape):
    n, h, w, cin, cout, k = shape
    x, wt, b = ternary((n, h, w, cin), 4), ternary((k, k, cin, cout), 5), ternary((cout,), 6)
    ref = T.conv2d(to64(x), to64(wt), to64(b)).numpy()
    assert_exact_conditions(T.conv2d(to64(np.abs(x)), to64(np.abs(wt)), to64(np.abs(b))).numpy(), ref, True)
    act = lrelu_f32(ref)
    pooled, idx = first_max_pool(act)
    assert_exact(pooled, T.max_pool2(to64(act)).numpy(), 'pooled')
    p_last, idx_last = first_max_pool(act, last=True)
    assert_exact(p_last, pooled, 'the maximum does not depend on the tie rule')
    assert (idx != idx_last).mean() > 0.02, 'integer data must make ties frequent'
    with pytest.raises(AssertionError):
        assert_exact(idx_last, idx, 'last maximum')
    # the routing of a pooled gradient follows the indices: autograd's max-pool picks the first maximum too
    gp = small_ints(pooled.shape, 7)
    a = to64(act).requires_grad_(True)
    (T.max_pool2(a) * to64(gp)).sum().backward()
    assert_exact(unpool(gp, idx), a.grad.numpy(), 'un-pooling')


def test_leaky_relu_is_one_float32_multiply():
    v = np.arange(-300, 301).astype(np.float64) * 2.0 ** -6
    got = lrelu_f32(v)
    assert got.dtype == np.float32
    assert np.array_equal(got[v > 0], v[v > 0].astype(np.float32))
    assert np.array_equal(got[v <= 0], (np.float32(0.2) * v[v <= 0].astype(np.float32)))
    assert not np.array_equal(got.astype(np.float64), np.where(v > 0, v, 0.2 * v))        # the float64 product is another number
    with pytest.raises(AssertionError):
        lrelu_f32(np.float64([1.0 + 2.0 ** -40]))


def test_conditions_hold_at_the_largest_k_of_the_matrix():
    """3x3 x 512 channels (the UNet's deepest level, 8 x 8 images): small_ints(3) for float32 outputs, ternary(1/4) for bf16."""
    n, h, w, c, k = 5, 8, 8, 512, 3
    for gen, stores_bf16 in ((small_ints, False), (ternary, True)):
        x, wt, b = gen((n, h, w, c), 11), gen((k, k, c, c), 12), gen((c,), 13)
        ref = T.conv2d(to64(x), to64(wt), to64(b)).numpy()
        absum = T.conv2d(to64(np.abs(x)), to64(np.abs(wt)), to64(np.abs(b))).numpy()
        assert_exact_conditions(absum, ref, stores_bf16)
        assert absum.max() < 2 ** 15 and (not stores_bf16 or np.abs(ref).max() <= 128)       # a wide margin, not a near miss
        assert_exact(_stand_in(x, wt, b), ref, 'largest K')
    with pytest.raises(AssertionError):                        # a case that is NOT exact is refused, not silently compared
        assert_exact_conditions(np.float64([2.0 ** 24]), np.zeros(1), False)
    with pytest.raises(AssertionError):
        assert_exact_conditions(np.float64([10.0]), np.float64([257.0]), True)
    assert_exact_conditions(np.float64([10.0 * 2.0 ** -6]), np.float64([256.0 * 2.0 ** -6]), True, scale=2.0 ** -6)
