"""
CPU self-tests of tests/operand_cases.py (no GPU): every builder runs and its own assertions hold; every comparison the GPU module
makes FAILS on the wrong variants (taps not flipped, ci / co swapped, truncation instead of round-to-nearest-even, padding left at
the fill byte, one 64-row block shifted, a policy that compares with <=); the sparse-image restatement is shown to be the operation
(a float64 GEMM over it reproduces oracle.tfops conv + util.unpool); and the cases are counted per route, the policy branches from
oracle.datafeed.Policy.
"""
import collections

import numpy as np
import pytest
import torch

import operand_cases as C
from oracle import datafeed as odf
from oracle import tfops as T
from util import assert_exact, small_ints, to64, unpool


def _fails(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


# ---- the comparison and the rounding
def test_bf16_bits_and_their_comparison():
    for name, bits, want in C.SPECIALS:
        got = C.bf16_bits(C.f32_bits([bits]))
        assert C.bf16_is_nan(got)[0] if want is None else got[0] == want, name
    a, _ = C.full_mantissa((1000,), 4)
    ref = C.bf16_bits(a)
    C.assert_bits_equal(ref, ref.copy())
    assert _fails(C.assert_bits_equal, C.bf16_bits(a, truncate=True), ref), 'truncation passes the comparison'
    nan = np.flatnonzero(C.bf16_is_nan(ref))
    assert len(nan) == 1
    other = ref.copy()
    other[nan[0]] = 0x7FFF                                     # another NaN: equal
    C.assert_bits_equal(other, ref)
    other[nan[0]] = 0x7F80                                     # an infinity where a NaN belongs
    assert _fails(C.assert_bits_equal, other, ref)
    zero = ref.copy()
    i = int(np.flatnonzero(ref == 0x8000)[0])
    zero[i] = 0x0000                                           # +0 where -0 belongs: the comparison is on bits
    assert _fails(C.assert_bits_equal, zero, ref)
    assert _fails(C.assert_all_written, np.array([1, 0xa5a5, 3], np.uint16))
    assert _fails(C.assert_all_written, np.array([0xa5a5a5a5], np.uint32).view(np.float32))


# ---- 1. weight images
def test_weight_image_cases_and_routes():
    names = [c['name'] for c in C.WIMG_LAYER_CASES]
    assert len(set(names)) == len(names)
    routes = collections.Counter(C.wimg_layer_route(c['kh'], c['kw'], c['cin'], c['cout'], c['mode']) + '-m{}'.format(c['mode'])
                                 for c in C.WIMG_LAYER_CASES)
    print('weight image routes:', dict(routes))
    for m in (0, 1):
        assert routes['one-workgroup-m{}'.format(m)] >= 3 and routes['several-workgroups-m{}'.format(m)] >= 3
        assert routes['second-trip-m{}'.format(m)] == 1
        cases = [c for c in C.WIMG_LAYER_CASES if c['mode'] == m]
        assert {(c['kh'], c['kw']) for c in cases} == set(C.WIMG_TAPS)
        padded = [c['cin'] if m == 0 else c['cout'] for c in cases]
        other = [c['cout'] if m == 0 else c['cin'] for c in cases]
        assert set(C.WIMG_PADDED) <= set(padded) and set(C.WIMG_OTHER) <= set(other)
        for kk in C.WIMG_TAPS:                                   # every kernel size with every padded length
            assert set(C.WIMG_PADDED) <= {(c['cin'] if m == 0 else c['cout']) for c in cases if (c['kh'], c['kw']) == kk}
    assert 5 * 5 * 160 * 160 == 640000 > C.WCAP
    planted = collections.Counter()
    for c in C.WIMG_LAYER_CASES:
        if c['cin'] * c['cout'] > 4096:
            continue                                             # (the two large ones: built on the GPU machine, and below)
        r = C.wimg_case(c)
        planted.update(r['planted'])
        assert r['ref'].dtype == np.uint16
    assert set(planted) == {s[0] for s in C.SPECIALS} and min(planted.values()) >= 5, planted
    # the batch table
    tiles = [e['tiles'] for e in C.WIMG_BATCH_ENTRIES]
    assert max(tiles) == 750 and sum(t > C.BATCH_WORKGROUPS for t in tiles) == 2 and min(tiles) == 1
    for m in (0, 1):
        rows = {(e['cout'] if m == 0 else e['cin']) for e in C.WIMG_BATCH_ENTRIES if e['mode'] == m}
        assert {1, 63, 64, 65} <= rows
    assert [c['n'] for c in C.WIMG_BATCH_CASES] == [len(C.WIMG_BATCH_ENTRIES), 1, 1, 40]
    assert C.batch_entries(C.WIMG_BATCH_CASES[1])[0]['tiles'] == 750 and len(C.batch_entries(C.WIMG_BATCH_CASES[3])) == 40
    sizes = [C.wimg_bytes(e['kh'], e['kw'], e['cin'], e['cout'], e['mode']) for e in C.WIMG_BATCH_ENTRIES]
    offs, total = C.batch_layout(sizes)
    assert all(o % 256 == 0 for o in offs) and all(offs[i] + sizes[i] + 256 <= offs[i + 1] for i in range(len(offs) - 1))
    assert total >= offs[-1] + sizes[-1] + 256


def test_weight_image_large_case_and_layout_statement():
    """The 640 000-element case builds in both modes; and the scatter agrees with the layout sentence of nimg.h read the other way
    round (a gather over the image's own index), on a ragged shape."""
    for m in (0, 1):
        c = [c for c in C.WIMG_LAYER_CASES if c['cin'] == 160 and c['mode'] == m][0]
        r = C.wimg_case(c)
        assert r['ref'].size == 25 * 160 * 160 and len(r['planted']) == len(C.SPECIALS)
    w, _ = C.full_mantissa((3, 1, 17, 5), 9)
    bits = C.bf16_bits(w).reshape(3, 17, 5)
    img0, img1 = C.wimg_reference(w, 0), C.wimg_reference(w, 1)
    assert img0.shape == (2, 3, 5, 16) and img1.shape == (1, 3, 17, 16)
    for chunk in range(2):
        for tap in range(3):
            for co in range(5):
                for k in range(16):
                    ci = 16 * chunk + k
                    want = bits[tap, ci, co] if ci < 17 else 0
                    assert img0[chunk, tap, co, k] == want or (C.bf16_is_nan(want) and C.bf16_is_nan(img0[chunk, tap, co, k]))
    for tap in range(3):
        for ci in range(17):
            for k in range(16):
                want = bits[2 - tap, ci, k] if k < 5 else 0
                assert img1[0, tap, ci, k] == want or (C.bf16_is_nan(want) and C.bf16_is_nan(img1[0, tap, ci, k]))


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('bug', ['noflip', 'swap', 'trunc', 'pad', 'rowblock'])
def test_weight_image_comparison_fails_on_wrong_images(mode, bug):
    shape = (3, 3, 70, 70) if bug in ('swap', 'rowblock') else ((3, 3, 17, 70) if mode == 0 else (3, 3, 70, 17))
    w, _ = C.full_mantissa(shape, 21)
    ref = C.wimg_reference(w, mode)
    C.assert_bits_equal(C.wimg_reference(w, mode), ref)
    if bug == 'noflip' and mode == 0:
        assert np.array_equal(C.wimg_reference(w, 0, bug='noflip'), ref)      # nothing to flip in mode 0: the same image
        return
    assert _fails(C.assert_bits_equal, C.wimg_reference(w, mode, bug=bug), ref), bug


# ---- 2. flip
def test_flip_cases():
    names = [c['name'] for c in C.FLIP_CASES]
    assert len(set(names)) == len(names)
    assert {(c['kh'], c['kw']) for c in C.FLIP_CASES} == {(1, 1), (2, 2), (3, 3), (5, 5), (1, 3)}
    small = [c for c in C.FLIP_CASES if c['cin'] <= 33]
    assert {(c['cin'], c['cout']) for c in small} == {(a, b) for a in C.FLIP_CH for b in C.FLIP_CH}
    assert sum('second-trip' in n for n in names) == 1 and 3 * 3 * 256 * 257 > 524288
    for c in C.FLIP_CASES:
        r = C.flip_case(c)
        assert r['ref'].shape == (c['kh'], c['kw'], c['cout'], c['cin'])
    w = C.flip_case(dict(kh=3, kw=3, cin=5, cout=5, name='x'))['w']
    ref = C.flip_reference(w)
    assert _fails(assert_exact, C.flip_reference(w, bug='noflip'), ref) and _fails(assert_exact, C.flip_reference(w, bug='swap'), ref)
    assert np.array_equal(ref, np.flip(w.reshape(9, 5, 5), axis=0).transpose(0, 2, 1).reshape(3, 3, 5, 5))


# ---- 3. the sparse image
def test_sparse_image_every_weight_lands_once_per_class():
    w, _ = C.full_mantissa((5, 5, 32, 8), 2, plant=False)
    hits = C.dgrad5s_reference(w, count=True)                           # (nt, chunk, wy, wx, plane, 128, 8)
    assert hits.max() == 1 and hits.sum() == 4 * w.size
    img = C.dgrad5s_reference(w)
    bits = C.bf16_bits(w)
    vals, counts = np.unique(img[hits == 1], return_counts=True)
    wv, wc = np.unique(bits, return_counts=True)
    assert np.array_equal(vals, wv) and np.array_equal(counts, 4 * wc), 'every weight lands exactly four times'
    # per class and channel: the 36 (window, position) slots of one co - 25 reached, 11 stay zero
    per = hits.reshape(1, 1, 3, 3, 4, 4, 32, 8)                         # (.., wy, wx, plane, cls, ci, j)
    for cls in range(4):
        for ci in (0, 31):
            for co in range(8):
                slots = []
                for wy in range(3):
                    for wx in range(3):
                        for pos in range(4):
                            k = 4 * co + pos
                            slots.append(per[0, 0, wy, wx, 2 * ((k >> 3) & 1) + (k >> 4), cls, ci, k & 7])
                assert len(slots) == 36 and sum(slots) == 25 and slots.count(0) == 11
    assert (img[hits == 0] == 0).all()
    assert C.dgrad5s_image_bytes(32, 8) == img.size * 2 == 9 * 4 * 128 * 16
    for cin, cout in C.DGRAD5S_REFUSED:
        assert C.dgrad5s_image_bytes(cin, cout) == 0
    assert 128 // 32 * (256 // 8) * 36864 > C.GCAP


def test_sparse_image_is_the_operation():
    """(cin, cout, h, w) = (32, 8, 4, 4), small integers: the dense GEMM over the restated image == the input gradient of
    oracle.tfops.conv2d (5 x 5, SAME) for the un-pooled gradient util.unpool(g, idx)."""
    w = small_ints((5, 5, 32, 8), 31, 3)
    g = small_ints((2, 2, 2, 8), 32, 4)
    idx = np.random.default_rng(33).integers(0, 4, size=g.shape).astype(np.uint8)
    dz = unpool(g, idx)
    x = torch.zeros((2, 4, 4, 32), dtype=torch.float64, requires_grad=True)
    y = T.conv2d(x, to64(w), None, 1, 'SAME')
    (y * to64(dz)).sum().backward()
    want = x.grad.numpy()
    assert np.abs(want).max() > 0
    got = C.dgrad5s_dense_gemm(C.dgrad5s_reference(w), g, idx)
    assert_exact(got, want, 'GEMM over the restated image')
    for bug in ('noflip', 'swap'):
        assert _fails(assert_exact, C.dgrad5s_dense_gemm(C.dgrad5s_reference(w, bug=bug), g, idx), want, bug), bug
    wf, _ = C.full_mantissa((5, 5, 32, 8), 5)
    assert _fails(C.assert_bits_equal, C.dgrad5s_reference(wf, bug='trunc'), C.dgrad5s_reference(wf))
    assert _fails(C.assert_bits_equal, C.dgrad5s_reference(wf, bug='pad'), C.dgrad5s_reference(wf))


def test_sparse_image_cases():
    for c in C.DGRAD5S_CASES[:3]:
        r = C.dgrad5s_case(c)
        assert r['ref'].size * 2 == C.dgrad5s_image_bytes(c['cin'], c['cout']) and len(r['planted']) == len(C.SPECIALS)
    assert [('second-trip' in c['name']) for c in C.DGRAD5S_CASES] == [False, False, False, True]


# ---- 4. space-to-depth builders
def test_s2d_weight_cases():
    names = [c['name'] for c in C.S2DW_CASES + C.S2DW_BWD_CASES]
    assert len(set(names)) == len(names)
    assert {c['c'] for c in C.S2DW_CASES} == {1, 3, 8, 64} and {c['cout'] for c in C.S2DW_CASES} == {1, 12, 128}
    for c in (1, 3, 8, 64):
        cps = {k['cp'] for k in C.S2DW_CASES if k['c'] == c}
        assert {4 * c, 4 * c + 4, C.ceil16(4 * c)} == cps
    assert sum('second-trip' in c['name'] for c in C.S2DW_CASES) >= 1 and 9 * 256 * 128 == 294912 > C.LCAP
    assert sum('second-trip' in c['name'] for c in C.S2DW_BWD_CASES) == 2 and 25 * 64 * 192 > C.LCAP
    for c in C.S2DW_CASES:
        if c['c'] * c['cout'] <= 1024:
            C.s2dw_case(c)
    for c in C.S2DW_BWD_CASES:
        r = C.s2dw_bwd_case(c)
        if c['acc']:
            assert not np.array_equal(r['ref'], C.s2d_weights_bwd_reference(r['dw3'], c['c']))
    c = dict(c=3, cp=16, cout=5, name='x')
    r = C.s2dw_case(c)
    for bug in ('noflip', 'swap', 'pad'):
        assert _fails(assert_exact, np.nan_to_num(C.s2d_weights_reference(r['w5'], 16, bug=bug).astype(np.float64), nan=-1.0), r['ref'], bug), bug
    # the statement as a convolution: a 5 x 5 stride-2 SAME convolution == the 3 x 3 stride-1 one over the space-to-depth image
    x = small_ints((1, 8, 8, 3), 3, 3)
    w5 = small_ints((5, 5, 3, 5), 4, 3)
    want = T.conv2d(to64(x), to64(w5), None, 2, 'SAME').numpy()
    xs = T.space_to_depth(to64(x), 2)
    got = T.conv2d(xs, to64(C.s2d_weights_reference(w5, 12)), None, 1, 'SAME').numpy()
    assert_exact(got, want, 'stride-2 5x5 as stride-1 3x3 over space-to-depth')


def test_s2d_affine_cases():
    names = [c['name'] for c in C.AFFINE_CASES]
    assert len(set(names)) == len(names)
    routes = collections.Counter(c['route'] + ('-second-trip' if 'second-trip' in c['name'] else '') for c in C.AFFINE_CASES)
    print('s2d2_affine routes:', dict(routes))
    assert routes['affine3'] >= 3 and routes['generic'] >= 6 and routes['affine3-second-trip'] == 1 and routes['generic-second-trip'] == 1
    assert 513 * 513 == 263169 > C.LCAP and 130 * 130 * 16 == 270400 > C.LCAP
    assert {c['ab'] for c in C.AFFINE_CASES if c['route'] == 'affine3'} == {0, 1, 2} == {c['ab'] for c in C.AFFINE_CASES if c['route'] == 'generic'}
    assert {c['c'] for c in C.AFFINE_CASES if c['route'] == 'generic'} == {1, 3, 4, 16}
    assert any(c['cp'] > 4 * c['c'] for c in C.AFFINE_CASES if c['route'] == 'generic')
    for c in C.AFFINE_CASES:
        if c['h'] > 100:
            continue
        r = C.affine_case(c)
        assert r['ref'].shape == (c['n'], c['h'] // 2, c['w'] // 2, c['cp']) and not r['ref'][..., 4 * c['c']:].any()
    a = [c for c in C.AFFINE_CASES if c['route'] == 'affine3' and c['h'] == 6 and c['ab'] == 1][0]
    g = [c for c in C.AFFINE_CASES if c['route'] == 'generic' and c['c'] == 3][0]
    ra, rg = C.affine_case(a), C.affine_case(g)
    assert np.array_equal(ra['x'], rg['x']) and g['ab'] == 1 and np.array_equal(ra['ref'][..., :12], rg['ref'][..., :12])
    for bug in ('swap', 'pad'):
        assert _fails(C.assert_bits_equal, C.affine_reference(ra['x'], 16, ra['a'], ra['b'], bug=bug), ra['ref']), bug
    for route in ('affine3', 'generic'):                       # (1/2, 1/4) is the pair that rounds: every route has it, small and large
        assert {c['h'] > 100 for c in C.AFFINE_CASES if c['route'] == route and c['ab'] == 2} == {False, True}
    rt = C.affine_case([c for c in C.AFFINE_CASES if c['route'] == 'affine3' and c['h'] == 6 and c['ab'] == 2][0])
    assert _fails(C.assert_bits_equal, C.affine_reference(rt['x'], 16, rt['a'], rt['b'], bug='trunc'), rt['ref'])
    x = ra['x']
    want = T.space_to_depth(to64(2.0 * x.astype(np.float64) - 1.0), 2).numpy()
    assert np.array_equal(C.bf16_values(ra['ref'][..., :12]).astype(np.float64), C.bf16_values(C.bf16_bits(want.astype(np.float32))))


# ---- 5. data feed
def test_stats_reference_and_cases():
    names = [c['name'] for c in C.STATS_CASES]
    assert len(set(names)) == len(names)
    assert {c['p'] for c in C.STATS_CASES} == {2, 10, 14, 96, 1024}
    assert {c['b'] * c['attempts'] for c in C.STATS_CASES} >= {1, 4096} and any(c['attempts'] == 1 for c in C.STATS_CASES)
    assert 2 * 3 == 6 < 64 and 10 * 15 == 150 < 256 < 14 * 21 == 294          # lane items of patch 2, 10, 14
    for c in C.STATS_CASES:
        r = C.stats_case(c)
        assert r['cand'].shape == (c['b'], c['attempts'], 2) and r['rgb'].shape[2] % 2 == 0
    r = C.stats_case(C.STATS_CASES[3])
    for i in range(3):
        for k in range(4):
            xx, yy = r['cand'][i, k]
            img = r['rgb'][r['image_idx'][i]]
            m, v = C.stats_reference(img, xx, yy, 96)
            nv, nm = odf.patch_stats(img, xx, yy, 96)
            assert abs(m - nm) < 1e-13 and abs(float(v) - nv) < 1e-13
            C.assert_stats(float(v), m, img, xx, yy, 96)                               # float(Fraction) is correctly rounded
            if v:
                assert _fails(C.assert_stats, float(v) * (1 + 2.0 ** -50), m, img, xx, yy, 96)
            assert _fails(C.assert_stats, float(v), np.nextafter(m, 1.0), img, xx, yy, 96)
            if r['image_idx'][i] == 4:
                assert v == 0 and m == 200 / 255
    big = C.stats_case(C.STATS_CASES[5])['rgb']
    m, v = C.stats_reference(big[0], 0, 0, 1024)
    assert m == 1.0 and v == 0
    m, v = C.stats_reference(big[1], 0, 0, 1024)
    assert m == 0.5 and v == C.Fraction(1, 4)
    S, SS, n = C.stats_exact(big[0], 0, 0, 1024)
    assert n * SS < 2 ** 64 and S * S < 2 ** 64 and n * n * 65025 > 2 ** 53           # the denominator does round: three roundings


def test_policy_cases_reach_their_branches():
    names = [c['name'] for c in C.SELECT_CASES]
    assert len(set(names)) == len(names)
    count = collections.Counter()
    for c in C.SELECT_CASES:
        r = C.select_case(c)
        count.update(r['seen'])
    print('policy branches (counted from oracle.datafeed.Policy):', dict(count))
    for b in C.SELECT_BRANCHES:
        assert count[b] >= 1, 'no case reaches ' + b
    assert {c['mode'] for c in C.SELECT_CASES} == {None, 'flat', 'flat-aggressive', 'dark-n-textured'}
    assert any(c['attempts'] == 1 for c in C.SELECT_CASES) and any(c['max_attempts'] == 1 for c in C.SELECT_CASES)
    assert any(c['max_attempts'] > c['attempts'] for c in C.SELECT_CASES)
    # the designed walk agrees with oracle.datafeed.select over an image-free stand-in: the same Policy, the same loop
    for mode in (None, 'flat', 'flat-aggressive', 'dark-n-textured'):
        for b in C.SELECT_BATCH_SIZES:
            r = C.select_batch(mode, b)
            assert r['cand'].shape == (b, 6, 2) and len({tuple(v) for v in r['cand'].reshape(-1, 2)}) == 6 * b
            assert len(r['want_xy']) == b and (b == 1 or len(set(r['want_used'])) > (1 if mode else 0))


def test_a_policy_with_inclusive_bounds_is_noticed():
    """Every boundary case (v exactly 0, 0.005, 0.01, 0.02; m exactly 0.35, 0.99; u exactly 0.5; equal variance) gives another answer
    under a policy that compares with <= / >=."""
    differs = []
    for c in C.SELECT_CASES:
        if C.select_reference(c, policy=C.PolicyWithInclusiveBounds)[0] != C.select_reference(c)[0]:
            differs.append(c['name'])
    print('cases a <= policy fails:', differs)
    for key in ('flat-v-exactly-0.01', 'flat-v-exactly-0.005', 'flat-coin-exactly-half', 'aggr-v-exactly-0.02', 'aggr-equal-variance',
                'dnt-reject-v-exactly-0-', 'dnt-reject-v-exactly-0.005', 'dnt-reject-m-exactly-0.35', 'dnt-reject-m-exactly-0.99'):
        assert any(key in n or n.startswith(key.rstrip('-')) for n in differs), key


def test_flat_patch_case_pins_both_choices():
    r = C.flat_patch_case()
    for ma in (2, 3):
        assert r['device'][ma]['used'] != [o[1] for o in r['oracle'][ma]]
    assert r['device'][3]['xy'] != [list(o[0]) for o in r['oracle'][3]]
    # the device's answer is the policy's answer on the EXACT statistics
    for ma in (2, 3):
        for i in range(4):
            case = dict(mode='dark-n-textured', max_attempts=ma, attempts=3, uni=[0.0] * 3, var=[], mean=[])
            for k in range(3):
                m, v = C.stats_reference(r['rgb'][i], r['cand'][i, k, 0], r['cand'][i, k, 1], r['p'])
                case['var'].append(float(v))
                case['mean'].append(m)
            (at, used), _ = C.select_reference(case)
            assert r['cand'][i, at].tolist() == r['device'][ma]['xy'][i] and used == r['device'][ma]['used'][i]
    # how often np.var of a flat patch is a positive residue
    for p in (32, 64):
        positive = sum(odf.patch_stats(np.full((p, p, 3), lv, np.uint8), 0, 0, p)[0] > 0 for lv in range(256))
        print('np.var > 0 on a flat {0} x {0} x 3 patch at {1} of 256 levels'.format(p, positive))
        assert positive > 100


def test_gather_cases():
    names = [c['name'] for c in C.GATHER_CASES]
    assert len(set(names)) == len(names)
    assert 6 * 512 * 768 > C.GCAP and 9 * 512 * 512 > C.GCAP
    for c in C.GATHER_CASES[:3]:
        r = C.gather_case(c)
        assert r['x'].shape == (c['b'], c['p'] // 2, c['p'] // 2, 4) and r['y'].shape == (c['b'], c['p'], c['p'], 3)
    r = C.gather_case(C.GATHER_CASES[0])
    assert len(np.unique(r['x'][0, ..., 2])) == 65536 and r['x'].max() == 1.0 and r['x'].min() == 0.0
    assert np.array_equal(r['y'][0], (r['rgb'][0].astype(np.float64) / 255).astype(np.float32))
