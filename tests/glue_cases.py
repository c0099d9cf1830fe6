"""
The cases of tests/test_gpu_glue_exact.py and their REFERENCE HALVES (float64, CPU only): the glue between the convolutions, the
image chain and the tail of the step - pooling and un-pooling, depth-to-space heads, the float32 transposed convolution, the
element-wise streams of ClassicISP / INet / the codec, dropout, the confusion matrix, the constrained-filter normalisation and the
SSIM / MS-SSIM family.  Each builder draws the operands, computes the float64 reference and asserts - on the reference alone - the
conditions under which the comparison means something (operand rule: DESIGN.md section 5).  The GPU tests call a builder and
compare the kernels with what it returns; tests/test_glue_helpers.py calls every builder without a GPU.

Operand rule.  Values are small integers or k / 256 (k / 4096 for the clip heads); scales and shifts are powers of two or dyadic
(scale 1, 1/2, 1/4; shift 0, 1/2); LeakyReLU runs with alpha = 1/4.  Every product and sum is then a float32 number (asserted with
is_f32 on the float64 reference), so a contraction to fma cannot matter.  bf16-stored operands keep at most 8 significant bits
after the sum and the x 1/4 (|g|, |add| <= 63; asserted with bf16_rne).  Routing kernels get operands whose elements all differ.
"""
import numpy as np
import torch

from oracle import tables as ot
from oracle import tfops as T

from util import (EXACT_SUM_LIMIT, assert_exact_conditions, assert_no_denormals, bf16_rne, depth_to_space2, distinct_bf16,
                  distinct_ints, dyadic_pixels, first_max_pool, is_f32, lane_complete_argmax, small_ints, space_to_depth2, unpool)

F32 = np.float32
ALPHA = 0.25                        # LeakyReLU slope of the exact cases (the library's default 0.2 is not dyadic)
CAP = 2048 * 256                    # grid cap of csrc/common.h grid_for (pointwise, pool, adam, losses): 2048 workgroups of 256 threads
LATENT_CAP = 1024 * 256             # ... of csrc/latent.hip (affine, lrelu, tanh, clip01, zero_insert2, d2s2_scale)
ISP_BIG = 8192 * 256 * 4 + 3        # above the 8192 workgroups of csrc/isp.hip, float4 items
PW_BIG = CAP + 3
STREAM_COUNTS = [0, 1, 3, 4, 5, 255, 256, 257, 4099]


def _seed(*parts):
    s = 29
    for p in parts:
        s = (s * 1000003 + (sum(ord(c) for c in p) if isinstance(p, str) else int(p))) % (2 ** 31 - 1)
    return s


def _names_unique(cases):
    names = [c['name'] for c in cases]
    assert len(set(names)) == len(names), 'duplicate case ids'
    return cases


def plant_zeros(a, seed):
    """Plant +0.0 and -0.0 (alternating) in about an eighth of the elements - both must take the alpha branch of `> 0`."""
    a = np.array(a, F32)
    flat = a.reshape(-1)
    where = np.flatnonzero(np.random.default_rng(seed).random(flat.size) < 0.125)
    flat[where[0::2]] = 0.0
    flat[where[1::2]] = -0.0
    return a


def plant_ties(x):
    """Plant, in every channel of the first image, a window with a 4-way, a 3-way and a 2-way tie (as far as the width allows);
    the 3- and 2-way ties have their first maximum at positions 1 and 2 - not where a last-maximum rule would put it."""
    x = np.array(x, F32)
    n, h, w, c = x.shape
    if h >= 2 and w >= 2:
        x[0, 0:2, 0:2] = 1.0
    if h >= 2 and w >= 4:
        x[0, 0, 2], x[0, 0, 3], x[0, 1, 2], x[0, 1, 3] = -1.0, 2.0, 2.0, 2.0
    if h >= 2 and w >= 6:
        x[0, 0, 4], x[0, 0, 5], x[0, 1, 4], x[0, 1, 5] = -2.0, 0.0, 1.0, 1.0
    return x


# ----------------------------------------------------------------------------------------------------------------------
# A. pooling
def _pool_values(shape, seed, big):
    """Small integers in [-2, 2] (ties in nearly every window); big: a non-repeating ramp pattern within +-125 (bf16 numbers)."""
    if not big:
        return small_ints(shape, seed, 2)
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    return ((i * 7919 + (i >> 9) * 31) % 251 - 125).astype(F32).reshape(shape)


MAXPOOL_CASES = []
for _c in (1, 3, 4, 6, 32):
    for _n, _h, _w in ((2, 6, 8), (1, 7, 8), (2, 6, 9), (1, 5, 7), (1, 2, 2)):
        MAXPOOL_CASES.append(dict(name='maxpool2<{}>-c{}-{}x{}x{}'.format(4 if _c % 4 == 0 else 1, _c, _n, _h, _w), n=_n, h=_h, w=_w,
                                  c=_c, bf16=False, big=False))
for _c in (8, 24):
    for _n, _h, _w in ((2, 6, 8), (1, 2, 2), (3, 4, 10)):
        MAXPOOL_CASES.append(dict(name='maxpool2-bf16-c{}-{}x{}x{}'.format(_c, _n, _h, _w), n=_n, h=_h, w=_w, c=_c, bf16=True, big=False))
MAXPOOL_CASES += [dict(name='maxpool2<1>-c1-1x1450x1451-above-cap', n=1, h=1450, w=1451, c=1, bf16=False, big=True),
                  dict(name='maxpool2<4>-c4-1x1451x1450-above-cap', n=1, h=1451, w=1450, c=4, bf16=False, big=True),
                  dict(name='maxpool2-bf16-c8-1x1450x1450-above-cap', n=1, h=1450, w=1450, c=8, bf16=True, big=True)]
_names_unique(MAXPOOL_CASES)


def tie_orders(act):
    """Set of the tie multiplicities (how many elements of a 2x2 window equal its maximum) that occur."""
    from util import pool_windows
    win = pool_windows(act)
    return set(np.unique((win == win.max(axis=-1, keepdims=True)).sum(axis=-1)).tolist())


def maxpool_case(case):
    n, h, w, c = case['n'], case['h'], case['w'], case['c']
    x = _pool_values((n, h, w, c), _seed('maxpool', case['name']), case['big'])
    x = x if case['big'] else plant_ties(x)
    he, we = h & ~1, w & ~1
    ref, _ = first_max_pool(x[:, :he, :we])
    v = c // (8 if case['bf16'] else (4 if c % 4 == 0 else 1))
    items = n * (h // 2) * (w // 2) * v
    assert (items > CAP) == case['big'], case['name']
    if w >= 8 and not case['big']:
        assert tie_orders(x[:, :he, :we]) >= {1, 2, 3, 4}, case['name'] + ': not every tie multiplicity occurs'
    if case['bf16']:
        assert np.array_equal(bf16_rne(x), x)
    return dict(x=x, ref=ref.astype(np.float64))


def maxpool_bwd_ref(dp, yact, add, mask, alpha=ALPHA, last=False, inclusive=False):
    """(first arg-max ? dp : 0) [+ add], [x 1 or alpha by yact > 0]; odd sizes pool VALID.  last / inclusive: the wrong rules of
    the self-test."""
    yact = np.asarray(yact)
    n, h, w, c = yact.shape
    he, we = h & ~1, w & ~1
    _, idx = first_max_pool(yact[:, :he, :we], last=last)
    dz = np.zeros(yact.shape, np.float64)
    dz[:, :he, :we] = unpool(np.asarray(dp, np.float64), idx)
    if add is not None:
        dz = dz + np.asarray(add, np.float64)
    if mask:
        pos = (yact >= 0) if inclusive else (yact > 0)
        dz = np.where(pos, dz, np.float64(alpha) * dz)
    return dz


MAXPOOL_BWD_CASES = []
for _kern, _c in (('f32<4>', 4), ('f32<4>', 8), ('f32<1>', 3), ('f32<1>', 1), ('bf16', 8), ('bf16', 24)):
    for _add in ('none', 'separate', 'inplace'):
        for _mask in (True, False):
            MAXPOOL_BWD_CASES.append(dict(name='maxpool2_bwd-{}-c{}-add_{}-{}'.format(_kern, _c, _add, 'mask' if _mask else 'nomask'),
                                          n=2, h=6, w=8, c=_c, bf16=_kern == 'bf16', add=_add, mask=_mask))
for _kern, _c in (('f32<4>', 4), ('f32<1>', 3)):
    for _h, _w in ((7, 8), (6, 9), (5, 7), (3, 3)):
        for _add, _mask in (('none', True), ('none', False), ('inplace', True), ('inplace', False), ('separate', True)):
            MAXPOOL_BWD_CASES.append(dict(name='maxpool2_bwd-{}-c{}-{}x{}-add_{}-{}'.format(_kern, _c, _h, _w, _add, 'mask' if _mask else 'nomask'),
                                          n=2, h=_h, w=_w, c=_c, bf16=False, add=_add, mask=_mask))
_names_unique(MAXPOOL_BWD_CASES)


def maxpool_bwd_case(case):
    n, h, w, c = case['n'], case['h'], case['w'], case['c']
    sd = _seed('maxpool_bwd', n, h, w, c, case['bf16'])
    yact = plant_ties(plant_zeros(small_ints((n, h, w, c), sd, 2), sd + 1))
    assert np.signbit(yact[yact == 0]).any() and not np.signbit(yact[yact == 0]).all(), 'both zeros are needed'
    if case['bf16']:
        dp = small_ints((n, h // 2, w // 2, c), sd + 2, 63)
        add = small_ints((n, h, w, c), sd + 3, 63)
    else:
        dp = distinct_ints((n, h // 2, w // 2, c), sd + 2, lo=1)
        add = -distinct_ints((n, h, w, c), sd + 3, lo=5000)
    add = None if case['add'] == 'none' else add
    raises = case['add'] == 'separate' and ((h | w) & 1) == 1
    ref = maxpool_bwd_ref(dp, yact, add, case['mask'])
    assert is_f32(ref), case['name']
    if case['bf16']:
        assert np.array_equal(bf16_rne(ref), ref), case['name'] + ': the result is not a bf16 number'
    if (h | w) & 1 and add is None:
        assert not ref[:, h & ~1:].any() and not ref[:, :, w & ~1:].any()
    if w >= 8:
        assert tie_orders(yact[:, :h & ~1, :w & ~1]) >= {1, 2, 3, 4}
    return dict(dp=dp, yact=yact, add=add, ref=ref, raises=raises)


UNPOOL_FORMS = {'x8': (True, True), '<true,true>': (True, True), '<true,false>': (True, False), '<false,true>': (False, True),
                '<false,false>': (False, False)}
UNPOOL_CASES = []
for _form in UNPOOL_FORMS:
    for _n, _ho, _wo in ((4, 1, 1), (2, 3, 7), (1, 7, 3)):
        _cs = (8, 16) if _form == 'x8' else ((12, 8) if _form == '<true,true>' else (4, 8))
        for _c in _cs:
            for _mask in (False, True):
                if (_form == 'x8' and _mask) or (_form == '<true,true>' and _c == 8 and not _mask):
                    continue                                # (bf16 -> bf16 without a mask at c % 8 == 0 IS the x8 form)
                UNPOOL_CASES.append(dict(name='unpool-{}-c{}-{}x{}x{}-{}'.format(_form, _c, _n, _ho, _wo, 'mask' if _mask else 'nomask'),
                                         form=_form, n=_n, ho=_ho, wo=_wo, c=_c, mask=_mask, big=False))
UNPOOL_CASES += [dict(name='unpool-x8-c8-1x727x727-above-cap', form='x8', n=1, ho=727, wo=727, c=8, mask=False, big=True),
                 dict(name='unpool-<false,false>-c4-1x727x727-mask-above-cap', form='<false,false>', n=1, ho=727, wo=727, c=4,
                      mask=True, big=True)]
_names_unique(UNPOOL_CASES)


def unpool_form(case):
    """The kernel ops.maxpool2_unpool reaches for (dtype of dp, dtype of out, mask, c) - nimg_maxpool2_unpool_ex restated."""
    in_b, out_b = UNPOOL_FORMS[case['form']]
    if in_b and out_b and not case['mask'] and case['c'] % 8 == 0:
        return 'x8'
    return '<{},{}>'.format('true' if in_b else 'false', 'true' if out_b else 'false')


def unpool_ref(dp, idx, pooled, mask, alpha=ALPHA, inclusive=False):
    g = np.asarray(dp, np.float64)
    if mask:
        pos = (np.asarray(pooled) >= 0) if inclusive else (np.asarray(pooled) > 0)
        g = np.where(pos, g, np.float64(alpha) * g)
    return unpool(g, idx)


def unpool_case(case):
    n, ho, wo, c = case['n'], case['ho'], case['wo'], case['c']
    sd = _seed('unpool', n, ho, wo, c)
    in_b, out_b = UNPOOL_FORMS[case['form']]
    assert unpool_form(case) == case['form'], case['name']
    assert (n * ho * wo * (c // (8 if case['form'] == 'x8' else 4)) > CAP) == case['big']
    dp = distinct_bf16((n, ho, wo, c), sd)                       # bf16 numbers: exact whichever way they are stored
    if not case['big']:
        assert len(np.unique(dp)) == dp.size
    idx = lane_complete_argmax((n, ho, wo, c), sd + 1)
    pooled = plant_zeros(small_ints((n, ho, wo, c), sd + 2, 2), sd + 3)
    assert (pooled == 0).any() and (pooled > 0).any() and (pooled < 0).any()
    ref = unpool_ref(dp, idx, pooled, case['mask'])
    assert is_f32(ref) and np.array_equal(bf16_rne(ref), ref), case['name'] + ': alpha * g is not a bf16 number'
    assert_no_denormals(ref, what=case['name'])
    return dict(dp=dp, idx=idx, pooled=pooled, ref=ref, in_bf16=in_b, out_bf16=out_b)


# ----------------------------------------------------------------------------------------------------------------------
# B. layout
CLIP_GRID = 2.0 ** -12
D2S_CONFIGS = [(1.0, 0.0, True), (1.0, 0.0, False), (0.5, 0.5, True), (0.25, 0.0, False)]
D2S_SHAPES = [('clip3', (2, 6, 5, 12)), ('clip3', (1, 1, 1, 12)), ('clip3', (1, 725, 725, 12))]
D2S_SHAPES += [('clip4', (2, 5, 7, 4 * _co)) for _co in (4, 8, 32, 128)] + [('clip4', (1, 363, 363, 16))]
D2S_SHAPES += [('generic', (2, 5, 7, 4 * _co)) for _co in (1, 2, 5)]
D2S_CASES = _names_unique([dict(name='d2s_{}-{}-scale{}-shift{}-{}'.format(_f, 'x'.join(map(str, _s)), _sc, _sh, 'clip' if _cl else 'noclip'),
                                form=_f, shape=_s, scale=_sc, shift=_sh, clip=_cl)
                           for _f, _s in D2S_SHAPES for _sc, _sh, _cl in D2S_CONFIGS])
D2S_BWD_CASES = _names_unique([dict(name='d2s_{}_bwd-{}-scale{}'.format(_f, 'x'.join(map(str, _s)), _sc), form=_f, shape=_s, scale=_sc)
                               for _f, _s in D2S_SHAPES for _sc in (1.0, 0.5)])


def d2s_form(shape):
    """nimg_d2s_clip_fwd / _bwd restated: the kernel family a shape (n, h, w, 4 co) reaches."""
    n, h, w, c4 = shape
    co = c4 // 4
    if co == 3:
        return 'clip3'
    if co % 4 == 0 and n * h * w * co < (1 << 32) - CAP:
        return 'clip4'
    return 'generic'


def d2s_items(shape):
    n, h, w, c4 = shape
    return {'clip3': n * h * w, 'clip4': n * h * w * (c4 // 4), 'generic': n * h * w * c4}[d2s_form(shape)]


def clip_head_values(shape, seed):
    """float32 values k / 4096 in [-1.5, 4.5], all different while the count allows it; the first elements are planted on the
    values that the four configurations map exactly onto 0 and 1, and one grid step on both sides of each."""
    count = int(np.prod(shape))
    lo, span = -6144, 24571                                  # (span: a prime below 6 * 4096)
    order = np.random.default_rng(seed).permutation(count) if count <= (1 << 22) else (np.arange(count) * 7919)
    k = lo + order % span
    plant = []
    for edge in (0, 4096, -4096, 16384):                     # x = 0, 1, -1, 4: scale x + shift lands on 0 or 1 for some configuration
        plant += [edge - 1, edge, edge + 1]
    k = k.astype(np.int64)
    if count >= 4 * len(plant):
        k[:len(plant)] = plant
    return (k * CLIP_GRID).astype(F32).reshape(shape)


def d2s_ref(x, scale, shift, clip, crd=False, swap_phase=False, exclusive=False):
    """clip(scale * depth_to_space(x) + shift, 0, 1), DCR order.  crd / swap_phase / exclusive: the wrong forms of the self-test
    (CRD channel order; row and column phase swapped; a clip that moves the ends off 0 and 1)."""
    x = np.asarray(x, np.float64)
    n, h, w, c4 = x.shape
    co = c4 // 4
    if crd:
        x = x.reshape(n, h, w, co, 4).transpose(0, 1, 2, 4, 3).reshape(n, h, w, c4)
    if swap_phase:
        x = x.reshape(n, h, w, 2, 2, co).transpose(0, 1, 2, 4, 3, 5).reshape(n, h, w, c4)
    pre = scale * depth_to_space2(x) + shift
    if not clip:
        return pre, pre
    out = np.clip(pre, 0.0, 1.0)
    if exclusive:
        out = np.clip(pre, CLIP_GRID, 1.0 - CLIP_GRID)
    return out, pre


def d2s_case(case):
    shape = case['shape']
    assert d2s_form(shape) == case['form'], case['name']
    x = clip_head_values(shape, _seed('d2s', *shape))
    ref, pre = d2s_ref(x, case['scale'], case['shift'], case['clip'])
    assert is_f32(pre) and is_f32(case['scale'] * x.astype(np.float64)), case['name'] + ': scale x + shift rounds'
    if x.size < 100000:
        assert np.array_equal(depth_to_space2(x), T.depth_to_space(torch.from_numpy(x), 2).numpy())
    if x.size >= 48:
        shares = [(pre == 0).any(), (pre == 1).any(), (pre < 0).any(), (pre > 1).any(), ((pre > 0) & (pre < 1)).any(),
                  (pre == -case['scale'] * CLIP_GRID).any() or case['scale'] != 1.0, (pre == 1 + case['scale'] * CLIP_GRID).any()]
        assert all(shares), '{}: the inputs do not land on 0, on 1 and on both sides of each ({})'.format(case['name'], shares)
    return dict(x=x, ref=ref)


def d2s_bwd_case(case):
    n, h, w, c4 = case['shape']
    assert d2s_form(case['shape']) == case['form']
    count = n * h * w * c4
    if count < (1 << 22):
        dy = distinct_ints((n, 2 * h, 2 * w, c4 // 4), _seed('d2s_bwd', n, h, w, c4), lo=-count // 2)
    else:
        dy = ((np.arange(count, dtype=np.int64) * 7919) % 1000003 - 500000).astype(F32).reshape(n, 2 * h, 2 * w, c4 // 4)
    ref = case['scale'] * space_to_depth2(dy.astype(np.float64))
    assert is_f32(ref)
    return dict(dy=dy, ref=ref)


D2S2_CASES = _names_unique([dict(name='d2s2_scale{}-c{}-cp{}-{}x{}x{}-scale{}'.format('3' if (_c, _cp) == (3, 16) else '', _c, _cp, _n, _hb, _wb, _sc),
                                 n=_n, hb=_hb, wb=_wb, c=_c, cp=_cp, scale=_sc)
                            for _c, _cp in ((3, 16), (1, 4), (1, 8), (4, 16), (4, 20), (3, 12))
                            for (_n, _hb, _wb), _sc in (((2, 3, 5), 1.0), ((1, 1, 1), 0.5), ((1, 7, 2), 0.25))]
                           + [dict(name='d2s2_scale3-c3-cp16-1x727x727-above-cap', n=1, hb=727, wb=727, c=3, cp=16, scale=0.5),
                              dict(name='d2s2_scale-c1-cp8-1x300x300-above-cap', n=1, hb=300, wb=300, c=1, cp=8, scale=0.5)])


def d2s2_case(case):
    n, hb, wb, c, cp = case['n'], case['hb'], case['wb'], case['c'], case['cp']
    count = n * hb * wb * cp
    if count < (1 << 22):
        xs = distinct_ints((n, hb, wb, cp), _seed('d2s2', n, hb, wb, c, cp), lo=-count // 2)
    else:
        xs = ((np.arange(count, dtype=np.int64) * 7919) % 1000003 - 500000).astype(F32).reshape(n, hb, wb, cp)
    ref = case['scale'] * depth_to_space2(xs[..., :4 * c].astype(np.float64))
    assert is_f32(ref)
    return dict(xs=xs, ref=ref)


ZERO_INSERT_CASES = _names_unique([dict(name='zero_insert2-c{}-{}x{}x{}'.format(_c, _n, _h, _w), n=_n, h=_h, w=_w, c=_c)
                                   for _c in (1, 3, 8) for _n, _h, _w in ((2, 3, 5), (1, 1, 1))]
                                  + [dict(name='zero_insert2-c3-1x150x151-above-cap', n=1, h=150, w=151, c=3)])


def zero_insert_case(case):
    n, h, w, c = case['n'], case['h'], case['w'], case['c']
    x = distinct_ints((n, h, w, c), _seed('zero_insert', n, h, w, c), lo=1)
    ref = np.zeros((n, 2 * h, 2 * w, c), np.float64)
    ref[:, ::2, ::2] = x
    return dict(x=x, ref=ref)


CONVT_PIX = {1: (1, 1, 1), 15: (1, 3, 5), 16: (2, 2, 4), 17: (1, 1, 17), 35: (1, 5, 7)}
CONVT_CASES = []
_i = 0
for _cin in (12, 24, 33, 64):
    for _cout in (4, 40, 65, 128):
        _npix = sorted(CONVT_PIX)[_i % 5]
        CONVT_CASES.append(dict(name='convt2x2_f32-cin{}-cout{}-npix{}-{}'.format(_cin, _cout, _npix, 'bias' if _i % 2 else 'nobias'),
                                cin=_cin, cout=_cout, npix=_npix, bias=bool(_i % 2), mode='f32'))
        _i += 1
for _npix in sorted(CONVT_PIX):
    for _bias in (True, False):
        CONVT_CASES.append(dict(name='convt2x2_f32-cin33-cout65-npix{}-{}-edge'.format(_npix, 'bias' if _bias else 'nobias'), cin=33,
                                cout=65, npix=_npix, bias=_bias, mode='f32'))
CONVT_CASES += [dict(name='convt2x2_f32-under-bf16-cin12-cout40-npix35-bias', cin=12, cout=40, npix=35, bias=True, mode='bf16'),
                dict(name='convt2x2_f32-under-bf16-cin24-cout4-npix17-bias', cin=24, cout=4, npix=17, bias=True, mode='bf16')]
_names_unique(CONVT_CASES)


def convt_case(case):
    n, h, w = CONVT_PIX[case['npix']]
    cin, cout = case['cin'], case['cout']
    sd = _seed('convt', cin, cout, case['npix'])
    x = small_ints((n, h, w, cin), sd, 3)
    wt = small_ints((2, 2, cout, cin), sd + 1, 3)
    wt.reshape(-1)[:] += (np.arange(wt.size) % 2 == 0) * (np.arange(wt.size) % 5 == 0)          # (breaks symmetries between the taps)
    b = small_ints((cout,), sd + 2, 5) if case['bias'] else None
    full = np.einsum('nyxc,ijoc->nyixjo', x.astype(np.float64), wt.astype(np.float64))
    ref = full.reshape(n, 2 * h, 2 * w, cout) + (0 if b is None else b.astype(np.float64))
    abs_sum = np.einsum('nyxc,ijoc->nyixjo', np.abs(x).astype(np.float64), np.abs(wt).astype(np.float64)).reshape(ref.shape) \
        + (0 if b is None else np.abs(b).astype(np.float64))
    assert_exact_conditions(abs_sum, ref, False, what=case['name'])
    if case['mode'] == 'bf16':
        assert cin % 8 != 0 or cout < 8, 'this shape would take the bf16 kernel'
    return dict(x=x, w=wt, b=b, ref=ref)


# ----------------------------------------------------------------------------------------------------------------------
# C. element-wise streams
def stream_ints(count, seed, m=100):
    return small_ints((count,), seed, m)


def add_case(count, n_inputs):
    xs = [stream_ints(count, _seed('add', count, i), 1000) for i in range(n_inputs)]
    ref = np.sum([x.astype(np.float64) for x in xs], axis=0) if count else np.zeros((0,), np.float64)
    assert is_f32(ref)
    return xs, ref


def lrelu_case(count, alpha):
    x = plant_zeros(stream_ints(count, _seed('lrelu', count), 100), _seed('lrelu0', count)) if count else np.zeros((0,), F32)
    dy = stream_ints(count, _seed('lrelu_dy', count), 100)
    fwd = np.where(x > 0, x.astype(np.float64), np.float64(alpha) * x)
    bwd = np.where(x > 0, dy.astype(np.float64), np.float64(alpha) * dy)
    relu = np.maximum(x.astype(np.float64), 0.0)
    assert is_f32(fwd) and is_f32(bwd)
    return dict(x=x, dy=dy, fwd=fwd, bwd=bwd, relu=relu, relu_bwd=np.where(x > 0, dy.astype(np.float64), 0.0))


def affine_case(count, a, b):
    x = dyadic_pixels((count,), _seed('affine', count)) * F32(4.0) - F32(2.0)
    ref = np.float64(a) * x + np.float64(b)
    assert is_f32(ref) and is_f32(np.float64(a) * x)
    clip = np.clip(x.astype(np.float64), 0.0, 1.0)
    if count >= 255:
        assert (x <= 0).any() and (x >= 1).any() and ((x > 0) & (x < 1)).any()
    return dict(x=x, ref=ref, clip=clip)


def mask_scale_case(count, scale):
    x = stream_ints(count, _seed('mask_scale', count), 1000)
    keep = np.random.default_rng(_seed('keep', count)).choice(np.array([0, 1, 2, 255], np.uint8), size=count)
    if count >= 255:
        assert set(np.unique(keep).tolist()) == {0, 1, 2, 255}
    prod = x * F32(scale)                                      # ONE float32 product, as the kernel forms it
    ref = np.where(keep != 0, prod, F32(0)).astype(np.float64)
    return dict(x=x, keep=keep, ref=ref, unscaled=np.where(keep != 0, x, 0).astype(np.float64))


def residual_case(count, alpha, with_f, clip):
    """y = [clip01](x - alpha f): x = k / 256 in [-0.5, 1.5], f = j / 64; alpha dyadic - x - alpha f is a float32 number, fused
    or not; the first elements are planted so that results of exactly 0 and exactly 1 occur."""
    sd = _seed('residual', count)
    x = (np.random.default_rng(sd).integers(-128, 385, size=count) / 256.0).astype(F32)
    f = (np.random.default_rng(sd + 1).integers(-64, 65, size=count) / 64.0).astype(F32)
    if count >= 5:
        f[:5] = [0.5, -0.5, 1.0, 0.0, 0.0]
        x[:5] = np.asarray([alpha * 0.5, 1.0 - alpha * 0.5, 1.0 + alpha, 0.0, 1.0], F32)
    prod = np.float64(alpha) * f
    pre = x.astype(np.float64) - (prod if with_f else 0.0)
    assert is_f32(prod) and is_f32(pre), 'x - alpha f rounds'
    ref = np.clip(pre, 0.0, 1.0) if clip else pre
    if count >= 255:
        assert (pre == 0).any() and (pre == 1).any() and (pre < 0).any() and (pre > 1).any()
    return dict(x=x, f=f if with_f else None, ref=ref)


RESIDUAL_BWD_COUNTS = [0, 1, 255, 257, 1024 * 256 + 5]


def residual_bwd_case(count, alpha, existing=None):
    dy = stream_ints(count, _seed('res_bwd', count), 3)
    f = stream_ints(count, _seed('res_bwd_f', count), 3)
    df = -np.float64(alpha) * dy
    terms = dy.astype(np.float64) * f
    dalpha = (0.0 if existing is None else float(existing)) - terms.sum()
    assert np.abs(terms).sum() + abs(existing or 0.0) < EXACT_SUM_LIMIT and is_f32(df)
    return dict(dy=dy, f=f, df=df, dalpha=np.float64(dalpha))


CONSTRAINED_CASES = _names_unique([dict(name='constrained-ks{}-c{}-strength{}'.format(_ks, _c, _s), ks=_ks, c=_c, strength=_s)
                                   for _ks in (3, 5, 7) for _c in (1, 3, 16) for _s in (100.0, 1.0)])


def constrained_reference(k, dnf, strength):
    """Forward and backward of oracle.tfops.constrained_kernel in float64 (autograd)."""
    ks, c = k.shape[0], k.shape[2]
    m = torch.tensor(ot.center_mask_2dfilter(ks, c), dtype=torch.float64)
    kt = torch.tensor(np.asarray(k), dtype=torch.float64).requires_grad_(True)
    nf = T.constrained_kernel(kt, m, strength)
    (nf * torch.tensor(np.asarray(dnf), dtype=torch.float64)).sum().backward()
    return nf.detach().numpy(), kt.grad.numpy() * (1 - m.numpy())


def constrained_case(case):
    """Integer kernels whose off-centre column sums are +-2^k: every division is exact."""
    ks, c, strength = case['ks'], case['c'], case['strength']
    sd = _seed('constrained', ks, c)
    k = small_ints((ks, ks, c, c), sd, 3)
    m = ot.center_mask_2dfilter(ks, c)
    for co in range(c):
        col = (k[..., co].astype(np.float64) * (1 - m[..., co]))
        target = (2.0 ** (co % 5)) * (1 if co % 2 == 0 else -1)
        k[0, 0, (co + 1) % c if c > 1 else 0, co] += target - col.sum()          # (an off-centre element: ks >= 3)
    sums = (k.astype(np.float64) * (1 - m)).sum(axis=(0, 1, 2))
    assert np.array_equal(np.abs(sums), 2.0 ** (np.arange(c) % 5)) and (c == 1 or (sums < 0).any())
    dnf = small_ints((ks, ks, c, c), sd + 1, 3)
    nf, dk = constrained_reference(k, dnf, strength)
    assert is_f32(nf) and is_f32(dk), case['name'] + ': the reference is not exact'
    dot = np.abs(dnf.astype(np.float64) * k * (1 - m)).sum(axis=(0, 1, 2))
    assert (strength * (dot + np.abs(dnf).max() * np.abs(sums)) * 1.0).max() < EXACT_SUM_LIMIT
    return dict(k=k, dnf=dnf, nf=nf, dk=dk)


CONFUSION_CASES = _names_unique([dict(name='confusion-k{}-n{}'.format(_k, _n), k=_k, n=_n) for _k in (1, 2, 7) for _n in (1, 255, 257, 5000)])


def confusion_ref(probs, labels, k, last=False):
    probs = np.asarray(probs)
    pred = (k - 1 - np.argmax(probs[:, ::-1], axis=1)) if last else np.argmax(probs, axis=1)
    conf = np.zeros((k, k), np.int64)
    ok = (labels >= 0) & (labels < k)
    np.add.at(conf, (labels[ok], pred[ok]), 1)
    return pred.astype(np.int32), conf


def confusion_case(case):
    k, n = case['k'], case['n']
    rng = np.random.default_rng(_seed('confusion', k, n))
    probs = (rng.integers(0, 9, size=(n, k)) / 8.0).astype(F32)            # quantised to 1/8: ties decide
    labels = rng.integers(-1, k + 1, size=n).astype(np.int32)              # -1 and k are ignored
    pred, conf = confusion_ref(probs, labels, k)
    if n >= 255 and k > 1:
        srt = np.sort(probs, axis=1)
        assert (srt[:, -1] == srt[:, -2]).any() and (labels == -1).any() and (labels == k).any()
        assert not np.array_equal(pred, confusion_ref(probs, labels, k, last=True)[0])
    return dict(probs=probs, labels=labels, pred=pred, conf=conf)


# ----------------------------------------------------------------------------------------------------------------------
# D. SSIM family
def gauss_window():
    """tf.image's 11 x 11 window (softmax of -(x^2 + y^2) / (2 sigma^2), sigma 1.5) ROUNDED TO float32 as the library holds it,
    returned as float64: the reference halves use the very weights the kernels read."""
    co = np.arange(11, dtype=np.float64) - 5.0
    g = -0.5 * (co[:, None] ** 2 + co[None, :] ** 2) / 1.5 ** 2
    g = np.exp(g - g.max())
    return (g / g.sum()).astype(F32).astype(np.float64)


def uniform_window(win=7):
    return np.full((win, win), 1.0 / (win * win))


def window_moments(a, b, wnd):
    """Five windowed moments (E a, E b, E aa, E bb, E ab) at the VALID positions: each (n, ho, wo, c), float64."""
    from numpy.lib.stride_tricks import sliding_window_view
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    k = wnd.shape[0]
    va = sliding_window_view(a, (k, k), axis=(1, 2))              # (n, ho, wo, c, k, k)
    vb = sliding_window_view(b, (k, k), axis=(1, 2))
    f = lambda v: np.einsum('nyxcij,ij->nyxc', v, wnd)
    return f(va), f(vb), f(va * va), f(vb * vb), f(va * vb)


def ssim_maps(a, b, mode='tf', max_val=1.0, population=None, const_max_val=None, wnd=None):
    """(ssim map, cs map, moments, (a1, a2, b1, b2)) in float64.  mode 'skimage': 7 x 7 uniform window and SAMPLE covariance
    (N / (N - 1)); 'tf': the Gaussian window and population moments.  population / const_max_val / wnd override single
    ingredients - the wrong forms of the self-test."""
    if wnd is None:
        wnd = uniform_window() if mode == 'skimage' else gauss_window()
    pop = (mode == 'tf') if population is None else population
    npix = float(wnd.size)
    covn = 1.0 if pop else npix / (npix - 1.0)
    mv = max_val if const_max_val is None else const_max_val
    c1, c2 = (0.01 * mv) ** 2, (0.03 * mv) ** 2
    ea, eb, eaa, ebb, eab = window_moments(a, b, wnd)
    a1, a2 = 2 * ea * eb + c1, 2 * covn * (eab - ea * eb) + c2
    b1, b2 = ea * ea + eb * eb + c1, covn * ((eaa - ea * ea) + (ebb - eb * eb)) + c2
    cs = a2 / b2
    return a1 * cs / b1, cs, (ea, eb, eaa, ebb, eab), (a1, a2, b1, b2)


def ssim_ref(a, b, mode='tf', max_val=1.0, **kw):
    """Per-image SSIM (n,) = the mean over positions and channels."""
    s = ssim_maps(a, b, mode, max_val, **kw)[0]
    return s.mean(axis=(1, 2, 3))


def ssim_planes_ref(y, t, max_val=1.0):
    """Per (image, channel) means of the SSIM and of the contrast-structure map (tf flavour): two (n, c) arrays."""
    s, cs = ssim_maps(y, t, 'tf', max_val)[:2]
    return s.mean(axis=(1, 2)), cs.mean(axis=(1, 2))


def derivative_maps(y, t, which, max_val=1.0, coef=1.0):
    """The three derivative maps (3, n, ho, wo, c) w.r.t. (E y, E yy, E yt), float64: which = 1 of the SSIM map, 2 of the
    contrast-structure map - the expressions of ssim_planes_kernel / ssim_loss_stats_kernel restated."""
    s, cs, (ey, et, _, _, _), (a1, a2, b1, b2) = ssim_maps(y, t, 'tf', max_val)
    if which == 1:
        inv = 1.0 / (b1 * b2)
        return coef * np.stack([2 * et * (a2 - a1) * inv - s * 2 * ey * (b2 - b1) * inv, -s / b2, 2 * a1 * inv])
    return coef * np.stack([(-2 * et * b2 + 2 * ey * a2) / (b2 * b2), -a2 / (b2 * b2), 2.0 / b2 + 0 * a2])


def maps_gradient(y, t, maps, gscale=1.0, coef=None):
    """d / dy through the transposed window: gscale * coef[n, c] * (G^T m0 + 2 y G^T m1 + t G^T m2), float64."""
    y, t, maps = np.asarray(y, np.float64), np.asarray(t, np.float64), np.asarray(maps, np.float64)
    wnd = gauss_window()
    n, h, w, c = y.shape
    ho, wo = h - 10, w - 10
    acc = np.zeros((3, n, h, w, c))
    for dy in range(11):
        for dx in range(11):
            acc[:, :, dy:dy + ho, dx:dx + wo, :] += wnd[dy, dx] * maps
    g = acc[0] + 2.0 * y * acc[1] + t * acc[2]
    if coef is not None:
        g = g * np.asarray(coef, np.float64).reshape(n, 1, 1, c)
    return gscale * g


def ssim_loss_ref(y, t, max_val=1.0, gscale=1.0):
    """(loss, gradient w.r.t. y) of mean_n 255 (1 - ssim_tf(y, t, max_val)_n), float64."""
    s = ssim_maps(y, t, 'tf', max_val)[0]
    n = s.shape[0]
    items = s[0].size
    loss = 255.0 - 255.0 * s.sum() / (n * items)
    maps = derivative_maps(y, t, 1, max_val, coef=-255.0 / (n * items))
    return loss, maps_gradient(y, t, maps, gscale), maps


def msssim_combine_ref(values, items):
    """nimg_msssim_combine in float64: ms = prod_k relu(v_k)^w_k per plane, loss = 255 (1 - mean ms), coef = d loss / d v_k / items_k."""
    v = np.asarray(values, np.float64)
    scales, planes = v.shape
    wts = np.asarray([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], F32).astype(np.float64)[:scales]
    ms = np.prod(np.maximum(v, 0.0) ** wts[:, None], axis=0)
    loss = 255.0 * (1.0 - ms.sum() / planes)
    with np.errstate(divide='ignore', invalid='ignore'):
        coef = np.where(v > 0, -255.0 / planes * wts[:, None] * ms[None, :] / v / np.asarray(items, np.float64)[:, None], 0.0)
    return loss, coef


def image_pair(n, h, w, c, seed, noise=0.08):
    """(y, t) float32 in [0, 1]: a natural-image-like target and a noisy copy of it."""
    from util import natural_images
    side = max(h, w, 8)
    t = np.stack([natural_images(n, side, side, seed + i)[:, :h, :w, i % 3] for i in range(c)], axis=-1).astype(F32)
    y = np.clip(t + noise * np.random.default_rng(seed + 99).uniform(-1, 1, size=t.shape), 0, 1).astype(F32)
    return y, t


def _ssim_shape_cases():
    out = []
    for mode, win in (('skimage', 7), ('tf', 11)):
        for (ho, wo), c, n in (((1, 1), 1, 1), ((1, 16), 3, 1), ((16, 17), 4, 3), ((17, 1), 3, 3), ((17, 17), 1, 1), ((16, 16), 3, 1),
                               ((5, 40), 3, 1)):
            out.append(dict(name='ssim<{}>-n{}-ho{}-wo{}-c{}'.format(win, n, ho, wo, c), mode=mode, n=n, h=ho + win - 1, w=wo + win - 1, c=c))
    out.append(dict(name='ssim<7>-n1-86x86x3-above-64-tiles', mode='skimage', n=1, h=86, w=86, c=3))
    out.append(dict(name='ssim<11>-n2-90x91x3-above-64-tiles', mode='tf', n=2, h=90, w=91, c=3))
    return out


SSIM_CASES = _names_unique(_ssim_shape_cases())


def ssim_tiles(case):
    win = 7 if case['mode'] == 'skimage' else 11
    ho, wo = case['h'] - win + 1, case['w'] - win + 1
    return ((ho + 15) // 16) * ((wo + 15) // 16) * case['c']


def ssim_case(case):
    y, t = image_pair(case['n'], case['h'], case['w'], case['c'], _seed('ssim', case['name']))
    return dict(a=y, b=t, ref=ssim_ref(y, t, case['mode']))


SSIM_LOSS_CASES = _names_unique(
    [dict(name='ssim_loss-n{}-{}x{}x{}-maxval{}'.format(_n, _h, _w, _c, _mv), n=_n, h=_h, w=_w, c=_c, max_val=_mv)
     for (_n, _h, _w, _c), _mv in (((1, 11, 11, 3), 1.0), ((2, 11, 12, 1), 1.0), ((1, 12, 21, 4), 1.0), ((2, 21, 22, 3), 1.0),
                                   ((1, 22, 11, 1), 1.0), ((3, 22, 22, 3), 1.0), ((1, 21, 12, 3), 255.0), ((1, 12, 12, 4), 1.0),
                                   ((1, 90, 90, 3), 1.0), ((2, 90, 90, 3), 255.0))])


def ssim_loss_case(case):
    y, t = image_pair(case['n'], case['h'], case['w'], case['c'], _seed('ssim_loss', case['name']))
    mv = case['max_val']
    if mv != 1.0:
        y, t = (y * F32(mv)).astype(F32), (t * F32(mv)).astype(F32)
    loss, grad, maps = ssim_loss_ref(y, t, mv)
    base = small_ints(y.shape, _seed('ssim_base', case['name']), 100).astype(np.float64) / (256.0 * mv)
    return dict(y=y, t=t, loss=loss, grad=grad, maps=maps, base=base.astype(F32), acc=base.astype(F32).astype(np.float64) + 0.25 * grad)


PLANES_CASES = _names_unique(
    [dict(name='ssim_planes-which{}-n{}-{}x{}x{}-{}'.format(_wh, _n, _h, _w, _c, _out), which=_wh, n=_n, h=_h, w=_w, c=_c, out=_out)
     for _wh, (_n, _h, _w, _c), _out in ((0, (2, 12, 13, 3), 'both'), (1, (2, 12, 13, 3), 'ssim'), (2, (2, 12, 13, 3), 'cs'),
                                         (1, (35, 12, 12, 2), 'both'), (2, (10, 12, 12, 7), 'cs'), (1, (1, 57, 58, 1), 'both'),
                                         (2, (1, 58, 57, 2), 'both'), (0, (1, 11, 11, 1), 'ssim'))])


def planes_case(case):
    y, t = image_pair(case['n'], case['h'], case['w'], case['c'], _seed('planes', case['name']))
    ms, mcs = ssim_planes_ref(y, t)
    maps = derivative_maps(y, t, case['which']) if case['which'] else None
    return dict(y=y, t=t, mean_ssim=ms, mean_cs=mcs, maps=maps)


COMBINE_PLANES = [1, 64, 65, 130]


def combine_case(planes, scales=5):
    rng = np.random.default_rng(_seed('combine', planes))
    v = (0.3 + 0.7 * rng.random((scales, planes))).astype(F32)
    if planes > 1:
        v[1, planes // 2] = 0.0                                  # relu(0) ^ w = 0: the whole plane's product is 0
        v[3, planes - 1] = -0.125                                # a negative contrast-structure mean is clamped to 0
    else:
        v[2, 0] = 0.0
    items = np.asarray([166.0 * 182, 78 * 86, 34 * 38, 12 * 14, 1.0], F32)[:scales]
    loss, coef = msssim_combine_ref(v, items)
    return dict(values=v, items=items, loss=loss, coef=coef)


def maps_grad_case(n=2, h=13, w=24, c=3):
    y, t = image_pair(n, h, w, c, _seed('maps_grad', n, h, w, c))
    maps = derivative_maps(y, t, 2).astype(F32)
    coef = (np.random.default_rng(5).uniform(-2, 2, size=(n, c))).astype(F32)
    ref = maps_gradient(y, t, maps, 0.5, coef)
    base = small_ints(y.shape, 11, 5)
    return dict(y=y, t=t, maps=maps, coef=coef, ref=ref, base=base, acc=base.astype(np.float64) + ref)


def maps_bound(ref64):
    """The bound of the float32 derivative maps: casts of float64 values - one rounding (2^-24 |ref|) with a factor 2 for the
    float64 summation order, plus an absolute 1e-12."""
    return 2.0 ** -23 * np.abs(np.asarray(ref64, np.float64)) + 1e-12
