"""
The helpers of the tail tests (tests/util.py, tests/tail_cases.py; used by tests/test_gpu_tail_exact.py), checked without a GPU -
the proof that the GPU tests can fail.  float32 numpy stand-ins take the place of the kernels: the honest one must pass every
comparison, and a loss accumulated in float32, a dropped ragged tail or last partial block, swapped halves of the s2d3 pixel, a
bias sum that skips the last channel chunk, a pooling backward without its / hw, an inclusive LeakyReLU mask, four wrong Adams
and a histogram that loses one workgroup's partial must each be rejected.  And the reference half of EVERY case of the GPU file
runs here, so its exactness conditions are asserted on this side too.
"""
import numpy as np
import pytest
import torch

from oracle import tfops as T

import tail_cases as C
from util import (assert_exact, depth_to_space2, is_f32, mask_f32, odd_part, pack_bits, pixel_pairs, space_to_depth2, to64)

F32 = np.float32


def _case(cases, name):
    return next(c for c in cases if c['name'] == name)


def test_every_reference_half_runs():
    for build, cases in ((C.loss_case, C.LOSS_CASES), (C.s2d3_case, C.S2D3_CASES + [C.S2D3_SWITCH, C.S2D3_SWITCH2]), (C.bias_case, C.BIAS_CASES),
                         (C.fan_linear_case, C.FAN_CASES), (C.fan_softmax_case, [c for c in C.FAN_CASES if c['c'] <= 256] + C.FAN_HW225),
                         (C.head_case, C.HEAD_CASES + [C.HEAD_ZERO_CASE]), (C.latent_case, C.LATENT_CASES + [C.LATENT_SWITCH]),
                         (C.latent_probe_case, C.LATENT_PROBE_CASES), (C.latent_rounding_case, C.LATENT_ROUNDING_CASES)):
        names = [c['name'] for c in cases]
        assert len(set(names)) == len(names), 'duplicate case ids'
        for case in cases:
            build(case)
    for count in C.POINT_COUNTS:
        C.pointwise_case(count, 2)
        C.lrelu_bwd_case(count)
    for count in C.ADDN_COUNTS:
        assert count % 4 == 0
        C.pointwise_case(count, 6)
    for count in C.ADAM_COUNTS:
        for gscale in (1.0, 0.5):
            C.adam_tier1_case(count, gscale)
        C.adam_tier2_case(count, 1e-3)
    for nblocks in C.HIST_BLOCKS:
        C.hist_case(nblocks)


def test_generators_and_the_divisibility_rule():
    a, b, j = pixel_pairs((5000,), 3)
    assert a.dtype == F32 and a.min() >= 0 and a.max() <= 1 and np.abs(j).max() == 127 and (j == 0).any()
    assert np.array_equal((a.astype(np.float64) - b) * 256, j) and np.array_equal(a * 256, np.rint(a * 256))
    assert [odd_part(n) for n in (1, 12, 96, 130050, 12582912)] == [1, 3, 3, 65025, 3]
    # the rule against the float32 arithmetic itself: gk is exact exactly at the counts the rule admits
    for kind in ('mse255', 'mae255'):
        for count in list(range(1, 700)) + [C.CAP - 256, C.CAP, C.CAP + 1, C.BENCH, 65025 * 32, 255 * 2 ** 13]:
            exact = float(C.kernel_gk(kind, 0.5, count)) * count == 0.5 * C.GK_CONST[kind]
            exact = exact and C.Fraction(float(C.kernel_gk(kind, 0.5, count))) * count == C.Fraction(C.GK_CONST[kind], 2)
            assert exact == C.grad_is_exact(kind, count), (kind, count)
    q = np.arange(2 * 3 * 4 * 12).reshape(2, 3, 4, 12)
    assert np.array_equal(space_to_depth2(depth_to_space2(q)), q)
    assert np.array_equal(space_to_depth2(depth_to_space2(q)), T.space_to_depth(torch.from_numpy(depth_to_space2(q)), 2).numpy())
    bits = np.zeros((2, 32), bool)
    bits[0, 0], bits[0, 31], bits[1, 5] = True, True, True
    assert pack_bits(bits).tolist() == [np.int32(-2 ** 31 + 1), 32]
    assert C.bias_blocks(511) == (1, 511, 0) and C.bias_blocks(1025) == (2, 513, 0) and C.bias_blocks(2048 * 512 + 1)[2] == 3
    assert [C.latent_route(K, v, u) for K, v, u in ((32, 50.0, True), (32, 50.0, False), (8, 2.0, False), (32, 2.5, False), (65, 50.0, True))] == \
        ['win32', 'fast32-m51', 'fast8-mint', 'generic64', 'generic128']


# ----------------------------------------------------------------------------------------------------------------------
def _loss_stand_in(kind, a, b, count, f32_sum=False, upto=None):
    """float32 element arithmetic like the kernels'; the sum in float64 (honest) or float32; upto: elements summed."""
    upto = count if upto is None else upto
    a, b = a[:upto], b[:upto]
    if kind == 'mse255':
        e = F32(255.0) * (a - b)
        terms = e.astype(np.float64) * e.astype(np.float64)
    elif kind == 'mae255':
        terms = np.abs(F32(255.0) * a - F32(255.0) * b).astype(np.float64)
    else:
        d = a - b
        terms = 0.5 * d.astype(np.float64) * d.astype(np.float64)
    s = np.float64(np.cumsum(terms.astype(F32), dtype=F32)[-1]) if f32_sum else terms.sum()       # (cumsum: one float32 accumulator)
    if kind == 'mse255':
        return F32(s / np.float64(count))
    return F32(s * (1.0 / np.float64(count))) if kind == 'mae255' else F32(s)


@pytest.mark.parametrize('kind', ['mse255', 'mae255', 'l2_loss'])
def test_loss_comparison_rejects_float32_sums_and_lost_elements(kind):
    case = _case(C.LOSS_CASES, '{}-n{}-loss'.format(kind, C.BENCH))
    r = C.loss_case(case)
    assert_exact([_loss_stand_in(kind, r['a'], r['b'], C.BENCH)], [r['loss']], 'honest')
    with pytest.raises(AssertionError):
        assert_exact([_loss_stand_in(kind, r['a'], r['b'], C.BENCH, f32_sum=True)], [r['loss']], 'float32 accumulator')
    cap = C.L2CAP if kind == 'l2_loss' else C.CAP
    for count, upto in ((cap + 1, cap), (257, 256), (C.DEEP[kind], C.DEEP[kind] - C.DEEP[kind] % 256)):         # ragged tail / last block
        r = C.loss_case(_case(C.LOSS_CASES, '{}-n{}-loss'.format(kind, count)))
        assert_exact([_loss_stand_in(kind, r['a'], r['b'], count)], [r['loss']], 'honest')
        if r['j'][upto:].any():
            with pytest.raises(AssertionError):
                assert_exact([_loss_stand_in(kind, r['a'], r['b'], count, upto=upto)], [r['loss']], 'dropped tail')


def test_loss_gradient_is_the_same_fused_or_not():
    for name in ('mse255-n{}-grad-acc'.format(65025 * 32), 'mae255-n{}-grad-acc'.format(255 * 2 ** 13), 'l2_loss-n257-grad-acc',
                 'mse255-n255-grad'):
        case = _case(C.LOSS_CASES, name)
        r = C.loss_case(case)
        d = r['a'] - r['b']
        if case['kind'] == 'l2_loss':
            g = F32(case['gscale']) * d
        else:
            gk = C.kernel_gk(case['kind'], case['gscale'], case['count'])
            g = gk * d if case['kind'] == 'mse255' else np.where(d > 0, gk, np.where(d < 0, -gk, F32(0)))
        unfused = g if r['existing'] is None else r['existing'] + g                  # two float32 roundings - none happens
        assert_exact(unfused, r['grad'], name)
        with pytest.raises(AssertionError):
            assert_exact(unfused * F32(1 + 2.0 ** -23), r['grad'], name)


def test_s2d3_comparison_rejects_swapped_halves():
    for case in (C.S2D3_SWITCH, _case(C.S2D3_CASES, 's2d3-pairs-w514-1x2x514-p3')):
        r = C.s2d3_case(case)
        gk = C.kernel_gk('mse255', case['gscale'], case['n'] * case['h'] * case['w'] * 12)
        acc = r['parts'][0].copy()
        for p in r['parts'][1:]:
            acc = acc + p
        img = (np.float64(gk) * (r['a'] - r['b']).astype(np.float64) + acc).astype(F32)           # one rounding: the fmaf
        got = space_to_depth2(img)
        assert_exact(got, r['dz'], 'honest')
        n, h, w, _ = got.shape
        swapped = got.reshape(n, h, w, 2, 6)[:, :, :, ::-1].reshape(n, h, w, 12)
        pixels = got.reshape(n, h, w, 2, 2, 3)[:, :, :, :, ::-1].reshape(n, h, w, 12)
        for wrong in (swapped, pixels, got[..., ::-1]):
            with pytest.raises(AssertionError):
                assert_exact(wrong, r['dz'], 'swapped')


def test_bias_comparison_rejects_a_skipped_channel_chunk():
    case = _case(C.BIAS_CASES, 'bias-generic-cout300-npix1025-acc')
    r = C.bias_case(case)
    honest = r['dz'].sum(axis=0, dtype=F32) + r['existing']
    assert_exact(honest, r['ref'], 'honest')
    wrong = honest.copy()
    wrong[256:] = r['existing'][256:]                       # the cb loop stopped after the first 256 channels
    with pytest.raises(AssertionError):
        assert_exact(wrong, r['ref'], 'skipped chunk')
    with pytest.raises(AssertionError):
        assert_exact(r['dz'][:-1].sum(axis=0, dtype=F32) + r['existing'], r['ref'], 'lost pixel')


def test_fan_comparison_rejects_a_missing_mean_and_an_inclusive_mask():
    case = _case(C.FAN_CASES, 'fan-vec-n5-hw64-c32-k5-parts16')
    r = C.fan_linear_case(case)
    g = (r['dlogits'] @ r['w'].T).astype(F32)
    full = np.broadcast_to(g[:, None, None, :], r['act'].shape)
    assert_exact(mask_f32(full / F32(case['hw']), r['act']), r['dact'], 'honest')
    assert_exact(r['act'].sum(axis=(1, 2), dtype=F32) * F32(1.0 / case['hw']), r['gap'], 'honest gap')
    with pytest.raises(AssertionError):
        assert_exact(mask_f32(full, r['act']), r['dact'], 'no / hw')
    with pytest.raises(AssertionError):
        assert_exact(r['dact_inclusive'], r['dact'], '>= 0 mask')
    with pytest.raises(AssertionError):
        assert_exact(r['act'][:, :-1].sum(axis=(1, 2), dtype=F32) / F32(case['hw']), r['gap'], 'lost pixel')
    z = C.head_case(C.HEAD_ZERO_CASE)
    pre32 = z['x'].reshape(-1, 64) @ z['w'].reshape(64, 64) + z['b']
    assert_exact(pack_bits((pre32 > 0).reshape(-1, 2, 32)), z['mask'], 'honest mask')
    with pytest.raises(AssertionError):
        assert_exact(pack_bits((pre32 >= 0).reshape(-1, 2, 32)), z['mask'], 'inclusive mask')
    assert_exact(z['mask_inclusive'], pack_bits((pre32 >= 0).reshape(-1, 2, 32)))


def test_adam_bound_passes_the_honest_kernel_and_rejects_four_wrong_ones():
    p0, grads, ref, pop = C.adam_tier2_case(4096, 1e-3)
    p, m, v, Ep, Em, Ev = ref

    def check(got):
        C.assert_within_bound(got[0], p, Ep, 'p')
        C.assert_within_bound(got[1], m, Em, 'm')
        C.assert_within_bound(got[2], v, Ev, 'v')

    check(C.adam_f32(p0, grads, 1e-3, 0.9, 0.999, 1e-7))
    for bug in ('eps_inside', 'no_eps', 'step_minus_1', 'betas_swapped'):
        with pytest.raises(AssertionError):
            check(C.adam_f32(p0, grads, 1e-3, 0.9, 0.999, 1e-7, bug=bug))
    # the bound is a rounding bound, not a tolerance: a few ulps of the parameter at most, nothing where the gradient is zero
    assert (Ep[pop == 2] <= 5 * 2.0 ** -24 * np.abs(p0[pop == 2]) * 1.0001).all() and (Ep <= 1e-6).all() and not Em[pop == 2].any()
    for gscale in (1.0, 0.5):
        p0, grads, ref = C.adam_tier1_case(1000, gscale)
        got = C.adam_f32(p0, grads, 1e-3, 0.5, 0.75, 1e-7, gscale)
        assert_exact(got[1], ref[1], 'tier 1 m')
        assert_exact(got[2], ref[2], 'tier 1 v')
        C.assert_within_bound(got[0], ref[0], ref[3], 'tier 1 p')


def test_histogram_closed_form_and_a_lost_partial():
    for nblocks in (17, 1024):
        r = C.hist_case(nblocks)
        ent, _ = T.entropy(to64(r['z']), to64(r['cb']))
        assert abs(float(ent) - r['entropy']) < 1e-9, 'the closed form is not the oracle\'s entropy'
        lat = T.soft_codebook(to64(r['z'][:2000]), to64(r['cb']))
        assert np.array_equal(lat.numpy().astype(F32), r['z'][:2000])
        lost = C.hist_case(nblocks, drop_block=nblocks // 2)['entropy']
        assert abs(lost - r['entropy']) > 1e-5, 'a lost workgroup partial would pass the 1e-5 comparison'
