"""
The helpers of the glue tests (tests/util.py, tests/glue_cases.py; used by tests/test_gpu_glue_exact.py), checked without a GPU -
the proof that the GPU tests can fail.  float32 numpy stand-ins take the place of the kernels: the honest one must pass every
comparison, and a last-maximum rule, an inclusive LeakyReLU mask, swapped byte lanes of an 8-channel granule, CRD in place of DCR,
swapped row and column phases, exclusive clip bounds, a dropped count % 4 tail, dropout without its scale, population in place of
sample covariance, c1 and c2 taken at the wrong max_val, the uniform window in place of the Gaussian one and a last arg-max must
each be rejected.  The reference half of EVERY case of the GPU file runs here, so its exactness conditions are asserted on this
side too, and the float64 SSIM restatements are anchored to oracle.tfops (ssim_tf, ssim_skimage, ssim_multiscale, autograd).
"""
import numpy as np
import pytest
import torch

from oracle import tfops as T

import glue_cases as C
from util import (assert_close, assert_exact, bf16_rne, depth_to_space2, distinct_bf16, distinct_ints, first_max_pool,
                  lane_complete_argmax, space_to_depth2, to64, unpool)

F32 = np.float32


def _case(cases, name):
    return next(c for c in cases if c['name'] == name)


def rejected(got, ref):
    with pytest.raises(AssertionError):
        assert_exact(got, ref)


def test_every_reference_half_runs():
    groups = ((C.maxpool_case, C.MAXPOOL_CASES), (C.maxpool_bwd_case, C.MAXPOOL_BWD_CASES), (C.unpool_case, C.UNPOOL_CASES),
              (C.d2s_case, C.D2S_CASES), (C.d2s_bwd_case, C.D2S_BWD_CASES), (C.d2s2_case, C.D2S2_CASES),
              (C.zero_insert_case, C.ZERO_INSERT_CASES), (C.convt_case, C.CONVT_CASES), (C.constrained_case, C.CONSTRAINED_CASES),
              (C.confusion_case, C.CONFUSION_CASES), (C.ssim_case, C.SSIM_CASES), (C.ssim_loss_case, C.SSIM_LOSS_CASES),
              (C.planes_case, C.PLANES_CASES))
    total = 0
    for build, cases in groups:
        for case in cases:
            build(case)
        total += len(cases)
    for count in C.STREAM_COUNTS + [C.PW_BIG]:
        for n_in in range(2, 8):
            C.add_case(count, n_in)
        for alpha in (C.ALPHA, 0.0):
            C.lrelu_case(count, alpha)
        for a, b in ((0.5, 0.5), (0.25, 0.0), (1.0, -0.5)):
            C.affine_case(count, a, b)
    for count in C.STREAM_COUNTS + [C.ISP_BIG]:
        for scale in (2.0, float(F32(1 / 0.7))):
            C.mask_scale_case(count, scale)
        for alpha in (0.25, 0.375):
            for with_f in (True, False):
                C.residual_case(count, alpha, with_f, True)
    for count in C.RESIDUAL_BWD_COUNTS:
        C.residual_bwd_case(count, 0.375)
        C.residual_bwd_case(count, 0.25, existing=-12.0)
    for planes in C.COMBINE_PLANES:
        C.combine_case(planes)
    C.maps_grad_case()
    assert total > 300


def test_routes_are_the_ones_the_ids_name():
    """The dispatch restated in glue_cases (unpool_form, d2s_form, items against the caps) puts every case on the kernel of its id."""
    for case in C.UNPOOL_CASES:
        assert C.unpool_form(case) == case['form']
    assert {c['form'] for c in C.UNPOOL_CASES} == set(C.UNPOOL_FORMS)
    for case in C.D2S_CASES + C.D2S_BWD_CASES:
        assert C.d2s_form(case['shape']) == case['form']
    above = [c for c in C.D2S_CASES if C.d2s_items(c['shape']) > C.CAP]
    assert {c['form'] for c in above} == {'clip3', 'clip4'}
    assert C.d2s_form((1, 1 << 15, 1 << 15, 16)) == 'generic' and C.d2s_form((1, 1 << 14, 1 << 15, 16)) == 'clip4'
    assert max(C.ssim_tiles(c) for c in C.SSIM_CASES if c['mode'] == 'skimage') > 64
    assert max(C.ssim_tiles(c) for c in C.SSIM_CASES if c['mode'] == 'tf') > 64
    assert any((c['h'] - 10) * (c['w'] - 10) * c['c'] > 64 * 256 for c in C.SSIM_LOSS_CASES)
    assert any(c['n'] * c['c'] > 64 for c in C.PLANES_CASES) and any((c['h'] - 10) * (c['w'] - 10) > 8 * 256 for c in C.PLANES_CASES)
    assert {c['which'] for c in C.PLANES_CASES} == {0, 1, 2}
    for case in C.CONVT_CASES:
        assert case['mode'] == 'f32' or case['cin'] % 8 != 0 or case['cout'] < 8
    assert {c['npix'] for c in C.CONVT_CASES} == set(C.CONVT_PIX) and all(np.prod(v) == k for k, v in C.CONVT_PIX.items())


def test_generators():
    a = distinct_ints((3, 5, 7), 1, lo=-50)
    assert a.dtype == F32 and len(np.unique(a)) == a.size and a.min() == -50
    b = distinct_bf16((2, 3, 5, 8), 2)
    assert np.array_equal(bf16_rne(b), b) and len(np.unique(b)) == b.size and (b < 0).any() and (b > 0).any()
    assert np.array_equal(bf16_rne(0.25 * b.astype(np.float64)), 0.25 * b.astype(np.float64))
    idx = lane_complete_argmax((4, 1, 1, 16), 3)
    assert idx.dtype == np.uint8 and idx.max() == 3
    z = C.plant_zeros(np.ones(1000, F32), 4)
    assert np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
    x = C.clip_head_values((2, 6, 5, 12), 5)
    assert len(np.unique(x)) == x.size and np.array_equal(x * 4096, np.rint(x * 4096))
    assert C.tie_orders(C.plant_ties(np.zeros((1, 2, 8, 1), F32) - 3 + np.arange(16, dtype=F32).reshape(1, 2, 8, 1) * 0)) >= {2, 3, 4}


# ----------------------------------------------------------------------------------------------------------------------
# pooling and un-pooling
def test_pooling_comparisons_reject_the_wrong_rules():
    case = _case(C.MAXPOOL_BWD_CASES, 'maxpool2_bwd-f32<4>-c4-add_separate-mask')
    r = C.maxpool_bwd_case(case)
    honest = C.maxpool_bwd_ref(r['dp'], r['yact'], r['add'], True).astype(F32)
    assert_exact(honest, r['ref'])
    rejected(C.maxpool_bwd_ref(r['dp'], r['yact'], r['add'], True, last=True).astype(F32), r['ref'])
    rejected(C.maxpool_bwd_ref(r['dp'], r['yact'], r['add'], True, inclusive=True).astype(F32), r['ref'])
    rejected(C.maxpool_bwd_ref(r['dp'], r['yact'], r['add'], True, alpha=0.2).astype(F32), r['ref'])
    # defect 1 restated: the in-place call that leaves the dropped row / column without its LeakyReLU' factor
    case = _case(C.MAXPOOL_BWD_CASES, 'maxpool2_bwd-f32<4>-c4-5x7-add_inplace-mask')
    r = C.maxpool_bwd_case(case)
    wrong = r['ref'].copy()
    wrong[:, 4:] = r['add'][:, 4:]
    wrong[:, :, 6:] = r['add'][:, :, 6:]
    rejected(wrong, r['ref'])
    # forward pooling: the arg-max of the two rules differs on the planted ties, the pooled VALUE does not
    x = C.maxpool_case(_case(C.MAXPOOL_CASES, 'maxpool2<4>-c4-2x6x8'))['x']
    assert not np.array_equal(first_max_pool(x)[1], first_max_pool(x, last=True)[1])


def _swap_lanes(a, i, j):
    a = np.array(a)
    a[..., [i, j]] = a[..., [j, i]]
    return a


def test_unpool_comparisons_reject_lane_swaps_and_the_inclusive_mask():
    for name in ('unpool-x8-c8-2x3x7-nomask', 'unpool-x8-c16-4x1x1-nomask', 'unpool-<true,true>-c12-2x3x7-mask'):
        case = _case(C.UNPOOL_CASES, name)
        r = C.unpool_case(case)
        honest = C.unpool_ref(r['dp'].astype(F32), r['idx'], r['pooled'], case['mask']).astype(F32)
        assert_exact(honest, r['ref'])
        # swapped byte lanes of the arg-max word, of the gradient, of the output - each inside one 8-channel granule
        rejected(C.unpool_ref(r['dp'], _swap_lanes(r['idx'], 0, 1), r['pooled'], case['mask']), r['ref'])
        rejected(C.unpool_ref(r['dp'], _swap_lanes(r['idx'], 3, 4), r['pooled'], case['mask']), r['ref'])
        rejected(C.unpool_ref(_swap_lanes(r['dp'], 2, 3), r['idx'], r['pooled'], case['mask']), r['ref'])
        rejected(_swap_lanes(r['ref'], 6, 7), r['ref'])
        # a phase swap: positions 1 and 2 of the window exchanged
        rejected(unpool(r['dp'].astype(np.float64), np.where(r['idx'] == 1, 2, np.where(r['idx'] == 2, 1, r['idx']))), r['ref']) \
            if not case['mask'] else None
        if case['mask']:
            rejected(C.unpool_ref(r['dp'], r['idx'], r['pooled'], True, inclusive=True), r['ref'])


# ----------------------------------------------------------------------------------------------------------------------
# layout
def test_layout_comparisons_reject_crd_phase_swaps_and_exclusive_bounds():
    for name in ('d2s_clip4-2x5x7x16-scale0.5-shift0.5-clip', 'd2s_generic-2x5x7x8-scale1.0-shift0.0-clip',
                 'd2s_clip3-2x6x5x12-scale1.0-shift0.0-clip'):
        case = _case(C.D2S_CASES, name)
        r = C.d2s_case(case)
        sc, sh = F32(case['scale']), F32(case['shift'])
        honest = np.clip(sc * depth_to_space2(r['x']) + sh, F32(0), F32(1)).astype(F32)
        assert_exact(honest, r['ref'])
        rejected(C.d2s_ref(r['x'], case['scale'], case['shift'], True, crd=True)[0], r['ref'])
        rejected(C.d2s_ref(r['x'], case['scale'], case['shift'], True, swap_phase=True)[0], r['ref'])
        rejected(C.d2s_ref(r['x'], case['scale'], case['shift'], True, exclusive=True)[0], r['ref'])
        rejected(C.d2s_ref(r['x'], case['scale'], 0.0 if case['shift'] else 0.5, True)[0], r['ref'])
    for name in ('d2s_clip4_bwd-2x5x7x16-scale0.5', 'd2s_generic_bwd-2x5x7x20-scale1.0'):
        case = _case(C.D2S_BWD_CASES, name)
        r = C.d2s_bwd_case(case)
        assert_exact((F32(case['scale']) * space_to_depth2(r['dy'])).astype(F32), r['ref'])
        n, h, w, c4 = case['shape']
        crd = r['ref'].reshape(n, h, w, 4, c4 // 4).transpose(0, 1, 2, 4, 3).reshape(n, h, w, c4)
        rejected(crd, r['ref'])
    case = _case(C.D2S2_CASES, 'd2s2_scale-c4-cp20-2x3x5-scale1.0')
    r = C.d2s2_case(case)
    rejected(depth_to_space2(r['xs'][..., 4:20]), r['ref'])            # (reads the padding channels)
    assert_exact(depth_to_space2(r['xs'][..., :16]), r['ref'])
    case = _case(C.ZERO_INSERT_CASES, 'zero_insert2-c3-2x3x5')
    r = C.zero_insert_case(case)
    wrong = np.zeros_like(r['ref'])
    wrong[:, 1::2, 1::2] = r['x']
    rejected(wrong, r['ref'])
    case = _case(C.CONVT_CASES, 'convt2x2_f32-cin33-cout65-npix17-bias-edge')
    r = C.convt_case(case)
    rejected(C.convt_case(dict(case, cin=33))['ref'] - r['b'], r['ref'])                     # the bias dropped
    short = np.einsum('nyxc,ijoc->nyixjo', r['x'][..., :32].astype(np.float64), r['w'][..., :32].astype(np.float64))
    rejected(short.reshape(r['ref'].shape) + r['b'], r['ref'])                              # the ragged cin chunk (33 = 32 + 1) dropped
    swapped = np.einsum('nyxc,ijoc->nyjxio', r['x'].astype(np.float64), r['w'].astype(np.float64))
    rejected(swapped.reshape(r['ref'].shape) + r['b'], r['ref'])                            # row and column tap exchanged


# ----------------------------------------------------------------------------------------------------------------------
# streams
def test_stream_comparisons_reject_a_dropped_tail_and_unscaled_dropout():
    for count in (5, 255, 257, 4099):
        r = C.residual_case(count, 0.375, True, True)
        honest = np.clip(r['x'] - F32(0.375) * r['f'], F32(0), F32(1)).astype(F32)
        assert_exact(honest, r['ref'])
        tail = honest.copy()
        tail[count & ~3:] = 0.0                                # the count % 4 tail never written
        if count & 3:
            rejected(tail, r['ref'])
        r = C.lrelu_case(count, C.ALPHA)
        honest = np.where(r['x'] > 0, r['x'], F32(C.ALPHA) * r['x']).astype(F32)
        assert_exact(honest, r['fwd'])
        tail = honest.copy()
        tail[count & ~3:] = 7.5                                # (stale memory)
        if count & 3:
            rejected(tail, r['fwd'])
    for scale in (2.0, float(F32(1 / 0.7))):
        r = C.mask_scale_case(4099, scale)
        assert_exact(np.where(r['keep'] != 0, r['x'] * F32(scale), F32(0)), r['ref'])
        rejected(r['unscaled'], r['ref'])                      # dropout without its scale
        rejected(np.where(r['keep'] == 1, r['x'] * F32(scale), F32(0)), r['ref'])          # keep bytes 2 and 255 taken as dropped
    r = C.mask_scale_case(4099, float(F32(1 / 0.7)))
    rejected((r['x'].astype(np.float64) * (1 / 0.7) * (r['keep'] != 0)), r['ref'])        # (a float64 product is NOT the reference)
    r = C.residual_bwd_case(1024 * 256 + 5, 0.375)
    assert r['dalpha'] == -float((r['dy'].astype(np.float64) * r['f']).sum())
    short = -float((r['dy'][:1024 * 256].astype(np.float64) * r['f'][:1024 * 256]).sum())
    assert short != r['dalpha']                                 # the second trip past RED_BLOCKS carries weight
    xs, ref = C.add_case(4099, 3)
    chain = (xs[0] + xs[1]) + xs[2]
    assert_exact(chain, ref)
    rejected(((xs[0] + xs[1]) + (xs[0] + xs[1])), ref)          # the pairwise fallback writing over an input that is `out`


def test_constrained_and_confusion_comparisons():
    case = _case(C.CONSTRAINED_CASES, 'constrained-ks5-c3-strength100.0')
    r = C.constrained_case(case)
    m = C.ot.center_mask_2dfilter(5, 3).astype(F32)
    k = r['k']
    df = (k * (1 - m)).sum(axis=(0, 1, 2), dtype=F32)
    honest = np.where(m > 0, F32(-100.0), F32(100.0) * k / df).astype(F32)
    assert_exact(honest, r['nf'])
    rejected(np.where(m > 0, F32(-100.0), F32(100.0) * k / k.sum(axis=(0, 1, 2), dtype=F32)), r['nf'])     # the centre left in the sum
    dot = (r['dnf'] * k * (1 - m)).sum(axis=(0, 1, 2), dtype=F32)
    dk = np.where(m > 0, F32(0), F32(100.0) * (r['dnf'] / df - dot / (df * df))).astype(F32)
    assert_exact(dk, r['dk'])
    case = _case(C.CONFUSION_CASES, 'confusion-k7-n5000')
    r = C.confusion_case(case)
    pred_last, conf_last = C.confusion_ref(r['probs'], r['labels'], 7, last=True)
    assert not np.array_equal(pred_last, r['pred']) and not np.array_equal(conf_last, r['conf'])
    assert r['conf'].sum() == ((r['labels'] >= 0) & (r['labels'] < 7)).sum() < 5000


# ----------------------------------------------------------------------------------------------------------------------
# SSIM family
def test_ssim_restatements_are_anchored_to_the_oracle():
    y, t = C.image_pair(2, 23, 30, 3, 7)
    ref_tf = T.ssim_tf(to64(y), to64(t)).numpy()
    assert np.abs(C.ssim_ref(y, t, 'tf') - ref_tf).max() < 1e-7          # (the float32-rounded window: not bit-equal)
    ref_sk = np.array([T.ssim_skimage(y[i], t[i]) for i in range(2)])
    assert np.abs(C.ssim_ref(y, t, 'skimage') - ref_sk).max() < 1e-12
    ref255 = T.ssim_tf(to64(y) * 255, to64(t) * 255, 255.0).numpy()
    assert np.abs(C.ssim_ref(255.0 * y.astype(np.float64), 255.0 * t.astype(np.float64), 'tf', 255.0) - ref255).max() < 1e-7
    ms, mcs = C.ssim_planes_ref(y, t)
    o_ms, o_cs = T._ssim_per_channel(to64(y), to64(t))
    assert np.abs(ms - o_ms.numpy()).max() < 1e-7 and np.abs(mcs - o_cs.numpy()).max() < 1e-7
    # the loss and its gradient against autograd through the oracle
    yt = to64(y).requires_grad_(True)
    ref = T.ssim_loss255(yt, to64(t))
    gref, = torch.autograd.grad(ref, [yt])
    loss, grad, _ = C.ssim_loss_ref(y, t)
    assert abs(loss - float(ref.detach())) < 1e-5
    assert_close(grad, gref.numpy(), 1e-9, 1e-6, what='SSIM gradient restated')
    # the contrast-structure maps against autograd of the per-channel cs mean
    yt = to64(y).requires_grad_(True)
    cs = T._ssim_per_channel(yt, to64(t))[1]
    coef = np.random.default_rng(3).uniform(-1, 1, size=(2, 3))
    (cs * to64(coef)).sum().backward()
    items = 13 * 20
    mine = C.maps_gradient(y, t, C.derivative_maps(y, t, 2), 1.0 / items, coef)
    assert_close(mine, yt.grad.numpy(), 1e-9, 1e-6, what='cs gradient restated')
    # the combination of the scales against the oracle's ssim_multiscale
    y, t = C.image_pair(1, 176, 176, 1, 9)
    vals = []
    a, b = to64(y), to64(t)
    for k in range(5):
        if k:
            a, b = T.avg_pool(a, 2), T.avg_pool(b, 2)
        s, cs = T._ssim_per_channel(a, b)
        vals.append((s if k == 4 else cs).numpy().reshape(-1))
    loss, _ = C.msssim_combine_ref(np.stack(vals), np.ones(5))
    assert abs(loss - float(T.msssim_loss255(to64(y), to64(t)))) < 1e-4          # (float32-rounded weights)


def test_ssim_comparisons_reject_the_wrong_ingredients():
    y, t = C.image_pair(2, 23, 30, 3, 7)
    ref = C.ssim_ref(y, t, 'skimage')
    assert np.abs(C.ssim_ref(y, t, 'skimage', population=True) - ref).max() > 1e-5          # population in place of sample covariance
    assert np.abs(C.ssim_ref(y, t, 'skimage', wnd=C.gauss_window()[2:9, 2:9] / C.gauss_window()[2:9, 2:9].sum()) - ref).max() > 1e-5
    ref = C.ssim_ref(y, t, 'tf')
    assert np.abs(C.ssim_ref(y, t, 'tf', population=False) - ref).max() > 1e-5
    assert np.abs(C.ssim_ref(y, t, 'tf', wnd=C.uniform_window(11)) - ref).max() > 1e-5      # the uniform window in place of the Gaussian
    y255, t255 = 255.0 * y.astype(np.float64), 255.0 * t.astype(np.float64)
    ref255 = C.ssim_ref(y255, t255, 'tf', 255.0)
    assert np.abs(ref255 - ref).max() < 1e-9
    assert np.abs(C.ssim_ref(y255, t255, 'tf', 255.0, const_max_val=1.0) - ref255).max() > 1e-5   # c1, c2 at the wrong max_val
    # constant images: the closed form of the GPU test
    p, q = 0.25, 0.625
    for mode in ('skimage', 'tf'):
        for mv in (1.0, 255.0):
            a, b = np.full((1, 12, 13, 2), p * mv), np.full((1, 12, 13, 2), q * mv)
            c1 = (0.01 * mv) ** 2
            want = (2 * p * q * mv * mv + c1) / ((p * p + q * q) * mv * mv + c1)
            wnd = C.uniform_window() if mode == 'skimage' else C.gauss_window() / C.gauss_window().sum()
            assert abs(C.ssim_ref(a, b, mode, mv, wnd=wnd)[0] - want) < 1e-9
            # a window that sums to 1 - 6e-9 (the float32 table as it is) leaves a variance residue that c2 amplifies: ops.ssim
            # normalises its separable factor for that reason
            assert mode == 'skimage' or 1e-7 < abs(C.ssim_ref(a, b, mode, mv)[0] - want) < 1e-6
    assert (C.ssim_ref(y, y, 'tf') == 1.0).all() or np.abs(C.ssim_ref(y, y, 'tf') - 1.0).max() < 1e-15
    # the bound of the derivative maps admits a float32 cast of the reference and rejects a relative error of 4 ulp
    maps = C.derivative_maps(y, t, 1)
    cast = maps.astype(F32).astype(np.float64)
    assert (np.abs(cast - maps) <= C.maps_bound(maps)).all()
    assert not (np.abs(cast * (1 + 2.0 ** -21) - maps) <= C.maps_bound(maps)).all()
    r = C.combine_case(65)
    assert (r['coef'][r['values'] <= 0] == 0).all() and np.isfinite(r['coef']).all() and (r['values'] <= 0).sum() == 2
