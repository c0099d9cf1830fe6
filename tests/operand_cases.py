"""
The cases of tests/test_gpu_operands_exact.py and their REFERENCE HALVES (numpy / Python integers, CPU only): the operand-preparing
kernels every convolution of a step and every batch pass through first - bf16 weight images (per layer, batched, registered),
flipped weights, the 2:4 sparse input-gradient image, the space-to-depth builders of the codec's strided layers, and the data feed
(patch statistics, sampling policy, gather).  Each builder draws the operands, computes the reference, and asserts - on the
reference alone - the conditions under which the comparison means something.  The GPU tests call a builder and compare the kernels
with what it returns, by equality; tests/test_operand_helpers.py calls every builder without a GPU, shows that each comparison fails
on the wrong variants (`bug=`), and counts the cases per route.

Every reference is written from the documented layout (include/nimg.h) as loops over the SOURCE index (tap, ci, co) - a scatter - and
never over the flat output index the kernels decode.
"""
from fractions import Fraction

import numpy as np

from oracle import datafeed as odf

from util import assert_no_denormals, bf16_rne, distinct_ints, small_ints

F32 = np.float32
FILL = 0xa5                          # every output buffer is pre-filled with this byte and over-allocated by GUARD bytes
GUARD = 256
WCAP = 2048 * 256                    # grid cap of weights_bf16_kernel and flip_weights_kernel
LCAP = 1024 * 256                    # ... of csrc/latent.hip
GCAP = 8192 * 256                    # ... of csrc/datafeed.hip and dgrad5s_weights_kernel
BATCH_WORKGROUPS = 384               # workgroups per table entry of weights_bf16_batch_kernel


def _seed(*parts):
    s = 29
    for p in parts:
        s = (s * 1000003 + (sum(ord(c) for c in p) if isinstance(p, str) else int(p))) % (2 ** 31 - 1)
    return s


def ceil16(n):
    return (n + 15) // 16 * 16


# ----------------------------------------------------------------------------------------------------------------------
# bf16 bits
def f32_bits(bits):
    return np.asarray(bits, np.uint32).view(F32)


# float32 values whose bf16 rounding is a decision: (name, float32 bits, bf16 bits wanted; None = any NaN)
SPECIALS = [('tie-to-even-down', 0x3F808000, 0x3F80), ('tie-to-even-up', 0x3F818000, 0x3F82), ('up-across-a-binade', 0x3FFFFFFF, 0x4000),
            ('largest-finite-to-inf', 0x7F7FFFFF, 0x7F80), ('plus-zero', 0x00000000, 0x0000), ('minus-zero', 0x80000000, 0x8000),
            ('plus-inf', 0x7F800000, 0x7F80), ('minus-inf', 0xFF800000, 0xFF80), ('nan', 0x7FC00001, None),
            ('negative-tie-to-even-up', 0xBF838000, 0xBF84)]


def bf16_is_nan(bits):
    bits = np.asarray(bits, np.uint16)
    return ((bits & 0x7F80) == 0x7F80) & ((bits & 0x007F) != 0)


def bf16_bits(a, truncate=False):
    """uint16 bf16 bit patterns of a float32 array rounded to nearest even (util.bf16_rne, torch's conversion); a NaN stays a NaN.
    truncate: the wrong rule of the self-test."""
    a = np.ascontiguousarray(np.asarray(a, F32))
    if truncate:
        return (a.view(np.uint32) >> 16).astype(np.uint16)
    with np.errstate(all='ignore'):
        return (bf16_rne(a).astype(F32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_values(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(F32)


def assert_bits_equal(got, ref, what=''):
    """THE comparison of every bf16 image: the same bit pattern in every element; where the reference is a NaN, any NaN."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.uint16 and ref.dtype == np.uint16 and got.shape == ref.shape, '{}: {} {} vs {} {}'.format(
        what, got.dtype, got.shape, ref.dtype, ref.shape)
    nan = bf16_is_nan(ref)
    bad = np.where(nan, ~bf16_is_nan(got), got != ref)
    if bad.any():
        i = np.argwhere(bad)
        first = ['{} got {:#06x} want {:#06x}'.format(tuple(int(v) for v in k), int(got[tuple(k)]), int(ref[tuple(k)])) for k in i[:8]]
        raise AssertionError('{}: {} of {} elements differ (index box {} .. {}); first: {}'.format(
            what, len(i), got.size, tuple(int(v) for v in i.min(axis=0)), tuple(int(v) for v in i.max(axis=0)), '; '.join(first)))


def assert_all_written(ref_bytes, what=''):
    """A reference in which no 16-bit word (bf16 images) / 32-bit word (float32 outputs) is the fill pattern: a buffer pre-filled
    with 0xa5 that EQUALS it has then been written in every element."""
    ref_bytes = np.ascontiguousarray(ref_bytes)
    pat = {2: 0xa5a5, 4: 0xa5a5a5a5, 8: 0xa5a5a5a5a5a5a5a5, 1: None}[ref_bytes.dtype.itemsize]
    assert pat is not None
    words = ref_bytes.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[ref_bytes.dtype.itemsize])
    assert not (words == pat).any(), what + ': the reference holds the fill pattern - an unwritten element would pass'


def full_mantissa(shape, seed, plant=True):
    """float32 operands with all 24 mantissa bits in use (so that the bf16 rounding is visible), normal, of both signs, with the
    SPECIALS planted at the front, as many as fit, starting at special (seed % 10).  -> (array, names of the planted specials)."""
    rng = np.random.default_rng(seed)
    count = int(np.prod(shape))
    a = (rng.standard_normal(count) * 2.0 ** rng.integers(-6, 7, size=count)).astype(F32)
    a[a == 0] = F32(1.0009765625)
    planted = []
    if plant:
        for k in range(min(count, len(SPECIALS))):
            name, bits, _ = SPECIALS[(seed + k) % len(SPECIALS)]
            a[k] = f32_bits([bits])[0]
            planted.append(name)
    finite = a[np.isfinite(a)]
    assert_no_denormals(finite, what='weights')
    return a.reshape(shape), planted


for _n, _b, _w in SPECIALS:                        # the planted values round as their names say (torch's conversion is the rule)
    _got = bf16_bits(f32_bits([_b]))[0]
    assert (bf16_is_nan(_got) if _w is None else _got == _w), (_n, hex(int(_got)))
assert bf16_bits(f32_bits([0x3F818000]), truncate=True)[0] == 0x3F81


# ----------------------------------------------------------------------------------------------------------------------
# 1. bf16 weight images (csrc/conv_bf16.hip)
def wimg_bytes(kh, kw, cin, cout, mode):
    rows, cols = (cout, cin) if mode == 0 else (cin, cout)
    return kh * kw * rows * ceil16(cols) * 2


def wimg_reference(w, mode, bug=None):
    """w (kh, kw, cin, cout) float32 -> uint16 image [chunk][tap][row][16] as include/nimg.h states it:
         mode 0  wb[ci / 16][tap][co][ci % 16]            = w[tap][ci][co]
         mode 1  wb[co / 16][taps - 1 - tap][ci][co % 16] = w[tap][ci][co]
    zero padding up to 16 channels.  bug: 'noflip', 'swap' (ci / co roles), 'trunc', 'pad' (padding left at the fill byte),
    'rowblock' (the second 64-row block shifted by one row) - the wrong variants of the self-test."""
    kh, kw, cin, cout = w.shape
    taps = kh * kw
    wt = np.asarray(w, F32).reshape(taps, cin, cout)
    bits = bf16_bits(wt, truncate=(bug == 'trunc'))
    rows, cols = (cout, cin) if mode == 0 else (cin, cout)
    assert bug != 'pad' or cols % 16, 'no padding at this shape'
    img = np.full((ceil16(cols) // 16, taps, rows, 16), 0xa5a5 if bug == 'pad' else 0, np.uint16)
    for tap in range(taps):
        for ci in range(cin):
            if mode == 0:
                if bug == 'swap' and cin == cout:
                    img[np.arange(cout) // 16, tap, ci, np.arange(cout) % 16] = bits[tap, ci, :]
                else:
                    img[ci // 16, tap, :, ci % 16] = bits[tap, ci, :]                 # all co
            else:
                t2 = tap if bug == 'noflip' else taps - 1 - tap
                co = np.arange(cout)
                if bug == 'swap' and cin == cout:
                    img[ci // 16, t2, co, ci % 16] = bits[tap, ci, :]
                else:
                    img[co // 16, t2, ci, co % 16] = bits[tap, ci, :]
    if bug == 'rowblock':
        assert rows > 65
        img[:, :, 64:min(128, rows), :] = np.roll(img[:, :, 64:min(128, rows), :], 1, axis=2)
    return img


def wimg_layer_route(kh, kw, cin, cout, mode):
    total = wimg_bytes(kh, kw, cin, cout, mode) // 2
    return 'one-workgroup' if total <= 256 else ('second-trip' if total > WCAP else 'several-workgroups')


def wimg_batch_tiles(kh, kw, cin, cout, mode):
    rows, cols = (cout, cin) if mode == 0 else (cin, cout)
    return (ceil16(cols) // 16) * kh * kw * ((rows + 63) // 64)


WIMG_TAPS = [(1, 1), (2, 2), (3, 3), (5, 5), (1, 3), (3, 1)]
WIMG_PADDED = [3, 4, 12, 16, 17, 33]               # length of the axis padded to 16 (cin in mode 0, cout in mode 1)
WIMG_OTHER = [1, 3, 32, 65]


def _wimg_shape(kh, kw, padded, other, mode):
    cin, cout = (padded, other) if mode == 0 else (other, padded)
    return dict(kh=kh, kw=kw, cin=cin, cout=cout, mode=mode)


WIMG_LAYER_CASES = []
for _m in (0, 1):
    for _i, (_kh, _kw) in enumerate(WIMG_TAPS):
        for _j, _p in enumerate(WIMG_PADDED):
            WIMG_LAYER_CASES.append(_wimg_shape(_kh, _kw, _p, WIMG_OTHER[(_i + _j) % 4], _m))
    for _o in WIMG_OTHER:                          # ... and every `other` length with a ragged and a full padded axis at 3 x 3
        WIMG_LAYER_CASES.append(_wimg_shape(3, 3, 17, _o, _m))
        WIMG_LAYER_CASES.append(_wimg_shape(1, 1, 16, _o, _m))
    WIMG_LAYER_CASES.append(dict(kh=5, kw=5, cin=160, cout=160, mode=_m))
_seen = set()
WIMG_LAYER_CASES = [c for c in WIMG_LAYER_CASES if not (tuple(sorted(c.items())) in _seen or _seen.add(tuple(sorted(c.items()))))]
for _c in WIMG_LAYER_CASES:
    _c['name'] = 'wimg-layer-m{mode}-{kh}x{kw}-cin{cin}-cout{cout}'.format(**_c) + '-' + wimg_layer_route(
        _c['kh'], _c['kw'], _c['cin'], _c['cout'], _c['mode'])

# the batch table: all of the above plus the 64-row tile edge (rows 1, 63, 64, 65) at a ragged and a full chunk
WIMG_BATCH_ENTRIES = [dict(c) for c in WIMG_LAYER_CASES]
for _m in (0, 1):
    for _r in (1, 63, 64, 65):
        for _kh, _p in ((1, 16), (3, 17)):
            WIMG_BATCH_ENTRIES.append(_wimg_shape(_kh, _kh, _p, _r, _m))
for _c in WIMG_BATCH_ENTRIES:
    _c['name'] = 'm{mode}-{kh}x{kw}-cin{cin}-cout{cout}'.format(**_c)
    _c['tiles'] = wimg_batch_tiles(_c['kh'], _c['kw'], _c['cin'], _c['cout'], _c['mode'])
WIMG_BATCH_CASES = [dict(name='wimg-batch-all-{}-entries'.format(len(WIMG_BATCH_ENTRIES)), first=0, n=len(WIMG_BATCH_ENTRIES)),
                    dict(name='wimg-batch-n1-more-than-384-tiles', first=None, n=1),            # the 750-tile entry alone
                    dict(name='wimg-batch-n1-one-tile', first=0, n=1),
                    dict(name='wimg-batch-n40', first=3, n=40)]


def wimg_case(c):
    """-> dict(w, ref (uint16 image, flat), planted)."""
    w, planted = full_mantissa((c['kh'], c['kw'], c['cin'], c['cout']), _seed('wimg', c['kh'], c['kw'], c['cin'], c['cout']))
    ref = wimg_reference(w, c['mode']).reshape(-1)
    assert ref.size * 2 == wimg_bytes(c['kh'], c['kw'], c['cin'], c['cout'], c['mode'])
    r = ref[~bf16_is_nan(ref)]
    assert_all_written(r, c['name'])
    return dict(w=w, ref=ref, planted=planted)


def batch_layout(sizes, align=256, gap=256):
    """Slot offsets of a table's images: 256-byte aligned, at least `gap` fill bytes between two slots.  -> (offsets, total)."""
    offs, at = [], 0
    for s in sizes:
        offs.append(at)
        at += -(-s // align) * align + gap
    return offs, at


def batch_entries(case):
    if case['first'] is None:
        big = [e for e in WIMG_BATCH_ENTRIES if e['tiles'] > BATCH_WORKGROUPS and e['mode'] == 0]
        return big[:1]
    return WIMG_BATCH_ENTRIES[case['first']:case['first'] + case['n']]


# ----------------------------------------------------------------------------------------------------------------------
# 2. nimg_conv_flip_weights (csrc/conv_mfma.hip)
def flip_reference(w, bug=None):
    """wt[taps - 1 - t][co][ci] = w[t][ci][co]; -> (kh, kw, cout, cin)."""
    kh, kw, cin, cout = w.shape
    taps = kh * kw
    src = np.asarray(w).reshape(taps, cin, cout)
    wt = np.zeros((taps, cout, cin), src.dtype)
    for t in range(taps):
        for ci in range(cin):
            if bug == 'swap' and cin == cout:
                wt[taps - 1 - t, ci, :] = src[t, ci, :]
            else:
                wt[t if bug == 'noflip' else taps - 1 - t, :, ci] = src[t, ci, :]
    return wt.reshape(kh, kw, cout, cin)


FLIP_CH = [1, 3, 32, 33]
FLIP_CASES = []
for _i, (_kh, _kw) in enumerate([(1, 1), (2, 2), (3, 3), (5, 5), (1, 3)]):
    for _j in range(4):                            # 4 of the 16 (cin, cout) pairs per kernel size: all 16 over (1,1) .. (5,5)
        _k = 4 * (_i % 4) + _j
        FLIP_CASES.append(dict(kh=_kh, kw=_kw, cin=FLIP_CH[_k // 4], cout=FLIP_CH[(_k + _k // 4) % 4]))
FLIP_CASES.append(dict(kh=3, kw=3, cin=256, cout=257))                  # 592 128 elements: above the 2048 x 256 cap
for _c in FLIP_CASES:
    _c['name'] = 'flip-{kh}x{kw}-cin{cin}-cout{cout}'.format(**_c) + ('-second-trip' if _c['kh'] * _c['kw'] * _c['cin'] * _c['cout'] > WCAP else '')


def flip_case(c):
    w = distinct_ints((c['kh'], c['kw'], c['cin'], c['cout']), _seed('flip', c['kh'], c['kw'], c['cin'], c['cout']))
    ref = flip_reference(w)
    assert len(np.unique(w)) == w.size
    assert_all_written(ref, c['name'])
    assert np.array_equal(flip_reference(ref), w), 'flipping twice with the roles swapped is not the identity'
    return dict(w=w, ref=ref)


# ----------------------------------------------------------------------------------------------------------------------
# 3. the 2:4 sparse input-gradient image (csrc/dgrad5s.hip)
def dgrad5s_image_bytes(cin, cout):
    return 0 if (cin <= 0 or cout <= 0 or cin % 32 or cout % 8) else (cin // 32) * (cout // 8) * 9 * 4 * 128 * 8 * 2


def dgrad5s_reference(w, bug=None, count=False):
    """w (5, 5, cin, cout) float32 -> uint16 image img[nt][chunk][wy][wx][plane][32 cls + ci % 32][8], built by a scatter: the
    weight (ky, kx, ci, co) serves output parity class cls = 2 ey + ex through the window (wy, wx) and the position (py, px) with
         ky = ey + 4 - 2 wy - py,   kx = ex + 4 - 2 wx - px,
    i.e. 2 wy + py = ey + 4 - ky in 0 .. 5 - one place per class (the slots no tap reaches stay zero); inside the instruction's K = 32 the element is
    k = 4 (co % 8) + 2 py + px = 16 (plane & 1) + 8 (plane >> 1) + j.  count=True: -> the number of writes per image element."""
    _, _, cin, cout = w.shape
    assert cin % 32 == 0 and cout % 8 == 0
    bits = bf16_bits(w, truncate=(bug == 'trunc'))
    img = np.full((cin // 32, cout // 8, 3, 3, 4, 128, 8), 0xa5a5 if bug == 'pad' else 0, np.uint16)      # 'pad': the unreached slots unwritten
    hits = np.zeros(img.shape, np.int32)
    ci, co = np.meshgrid(np.arange(cin), np.arange(cout), indexing='ij')
    for ky in range(5):
        for kx in range(5):
            for cls in range(4):
                ey, ex = (cls >> 1, cls & 1) if bug != 'swap' else (cls & 1, cls >> 1)
                sy, sx = ey + 4 - ky, ex + 4 - kx
                if bug == 'noflip':
                    sy, sx = ey + ky, ex + kx
                wy, py, wx, px = sy >> 1, sy & 1, sx >> 1, sx & 1
                k = 4 * (co % 8) + 2 * py + px
                j, hb, part = k & 7, (k >> 3) & 1, k >> 4
                at = (ci // 32, co // 8, wy, wx, 2 * hb + part, 32 * cls + ci % 32, j)
                img[at] = bits[ky, kx]
                np.add.at(hits, at, 1)
    return hits if count else img


def dgrad5s_dense_gemm(img, g, idx):
    """A float64 GEMM over the restated image, the dense stand-in of the sparse product: g (n, hp, wp, cout) pooled gradient, idx its
    arg-max bytes -> din (n, 2 hp, 2 wp, cin).  A[(a, b)][(chunk, wy, wx, k)] = g[a + wy - 1][b + wx - 1][8 chunk + k / 4] where the
    arg-max is position k % 4 (else 0, and 0 outside the image); B = the image; column 32 cls + ci of the product is pixel
    (2 a + cls / 2, 2 b + cls % 2), channel ci."""
    nt, chunks = img.shape[0], img.shape[1]
    vals = bf16_values(img).astype(np.float64)
    n, hp, wp, cout = g.shape
    assert cout == 8 * chunks
    din = np.zeros((n, 2 * hp, 2 * wp, 32 * nt))
    gpad = np.zeros((n, hp + 2, wp + 2, cout))
    ipad = np.full((n, hp + 2, wp + 2, cout), 255, np.int64)
    gpad[:, 1:-1, 1:-1], ipad[:, 1:-1, 1:-1] = g, idx
    for t in range(nt):
        for a in range(hp):
            for b in range(wp):
                acc = np.zeros((n, 128))
                for chunk in range(chunks):
                    for wy in range(3):
                        for wx in range(3):
                            gv, iv = gpad[:, a + wy, b + wx, 8 * chunk:8 * chunk + 8], ipad[:, a + wy, b + wx, 8 * chunk:8 * chunk + 8]
                            A = np.zeros((n, 32))
                            for k in range(32):
                                A[:, k] = np.where(iv[:, k >> 2] == (k & 3), gv[:, k >> 2], 0.0)
                            B = np.zeros((32, 128))
                            for plane in range(4):
                                for j in range(8):
                                    B[16 * (plane & 1) + 8 * (plane >> 1) + j] = vals[t, chunk, wy, wx, plane, :, j]
                            acc += A @ B
                for cls in range(4):
                    din[:, 2 * a + (cls >> 1), 2 * b + (cls & 1), 32 * t:32 * t + 32] = acc[:, 32 * cls:32 * cls + 32]
    return din


DGRAD5S_CASES = [dict(cin=32, cout=8), dict(cin=64, cout=16), dict(cin=32, cout=64), dict(cin=128, cout=256)]
for _c in DGRAD5S_CASES:
    _c['name'] = 'dgrad5s-cin{cin}-cout{cout}'.format(**_c) + ('-second-trip' if dgrad5s_image_bytes(_c['cin'], _c['cout']) // 2 > GCAP else '')
DGRAD5S_REFUSED = [(31, 8), (32, 7), (48, 8), (32, 12), (0, 8), (32, 0)]


def dgrad5s_case(c):
    w, planted = full_mantissa((5, 5, c['cin'], c['cout']), _seed('dgrad5s', c['cin'], c['cout']))
    ref = dgrad5s_reference(w)
    assert ref.size * 2 == dgrad5s_image_bytes(c['cin'], c['cout'])
    assert_all_written(ref[~bf16_is_nan(ref)], c['name'])
    return dict(w=w, ref=ref.reshape(-1), planted=planted)


# ----------------------------------------------------------------------------------------------------------------------
# 4. space-to-depth builders (csrc/latent.hip)
def s2d_weights_reference(w5, cp, bug=None, count=False):
    """w3[dy][dx][(2 pr + pc) c + ci][co] = w5[2 dy + pr - 1][2 dx + pc - 1][ci][co], zero elsewhere; -> (3, 3, cp, cout)."""
    _, _, c, cout = w5.shape
    assert cp >= 4 * c
    w3 = np.zeros((3, 3, cp, cout), w5.dtype)
    if bug == 'pad':
        w3.view(np.uint8)[...] = FILL
        w3[:, :, :4 * c] = 0
    hits = np.zeros((5, 5), np.int32)
    for dy in range(3):
        for dx in range(3):
            for pr in range(2):
                for pc in range(2):
                    ky, kx = 2 * dy + pr - 1, 2 * dx + pc - 1
                    if bug == 'noflip':
                        ky, kx = 4 - ky, 4 - kx
                    if 0 <= ky <= 4 and 0 <= kx <= 4:
                        ph = (2 * pc + pr) if bug == 'swap' else (2 * pr + pc)
                        w3[dy, dx, ph * c:(ph + 1) * c, :] = w5[ky, kx]
                        hits[ky, kx] += 1
    return hits if count else w3


def s2d_weights_bwd_reference(dw3, c, existing=None):
    """dw5[ky][kx][ci][co] (+)= dw3[(ky + 1) / 2][(kx + 1) / 2][(2 pr + pc) c + ci][co], pr = (ky + 1) % 2 - the gather back."""
    cout = dw3.shape[3]
    dw5 = np.zeros((5, 5, c, cout), np.float64) if existing is None else np.asarray(existing, np.float64).copy()
    for dy in range(3):
        for dx in range(3):
            for pr in range(2):
                for pc in range(2):
                    ky, kx = 2 * dy + pr - 1, 2 * dx + pc - 1
                    if 0 <= ky <= 4 and 0 <= kx <= 4:
                        dw5[ky, kx] += dw3[dy, dx, (2 * pr + pc) * c:(2 * pr + pc + 1) * c, :]
    return dw5


def _cps(c):
    return sorted({4 * c, 4 * c + 4, ceil16(4 * c)})


S2DW_CASES = [dict(c=c, cp=cp, cout=cout) for c in (1, 3, 8, 64) for cp in _cps(c) for cout in (1, 12, 128)]
for _c in S2DW_CASES:
    _c['name'] = 's2dw-c{c}-cp{cp}-cout{cout}'.format(**_c) + ('-second-trip' if 9 * _c['cp'] * _c['cout'] > LCAP else '')
S2DW_BWD_CASES = [dict(c=c, cp=cp, cout=cout, acc=acc) for (c, cp, cout) in ((1, 4, 1), (3, 16, 12), (8, 36, 5), (64, 256, 192))
                  for acc in (0, 1)]
for _c in S2DW_BWD_CASES:
    _c['name'] = 's2dw-bwd-c{c}-cp{cp}-cout{cout}-acc{acc}'.format(**_c) + ('-second-trip' if 25 * _c['c'] * _c['cout'] > LCAP else '')


def s2dw_case(c):
    w5 = distinct_ints((5, 5, c['c'], c['cout']), _seed('s2dw', c['c'], c['cout']))
    ref = s2d_weights_reference(w5, c['cp'])
    assert (s2d_weights_reference(w5, c['cp'], count=True) == 1).all()
    vals, counts = np.unique(ref[ref != 0], return_counts=True)
    assert len(vals) == w5.size and (counts == 1).all(), 'each w5 element must appear exactly once in w3'
    assert np.array_equal(s2d_weights_bwd_reference(ref, c['c']), w5)
    assert not ref[:, :, 4 * c['c']:].any()
    assert_all_written(ref, c['name'])
    return dict(w5=w5, ref=ref)


def s2dw_bwd_case(c):
    dw3 = small_ints((3, 3, c['cp'], c['cout']), _seed('s2dwb', c['c'], c['cout']), 50)
    assert c['cp'] == 4 * c['c'] or dw3[:, :, 4 * c['c']:].any(), 'non-zero padding channels: they must be ignored'
    existing = small_ints((5, 5, c['c'], c['cout']), _seed('s2dwe', c['c'], c['cout']), 50) + F32(0.5)
    ref = s2d_weights_bwd_reference(dw3, c['c'], existing if c['acc'] else None)
    assert_all_written(ref.astype(F32), c['name'])
    return dict(dw3=dw3, existing=existing, ref=ref)


AFFINE_AB = [(1.0, 0.0), (2.0, -1.0), (0.5, 0.25)]
# (route, n, h, w, c, cp)
_AFF = [('affine3', 1, 2, 2, 3, 16), ('affine3', 1, 6, 10, 3, 16), ('affine3', 3, 2, 6, 3, 16), ('affine3', 1, 1026, 1026, 3, 16),
        ('generic', 1, 6, 10, 3, 32), ('generic', 2, 4, 6, 1, 4), ('generic', 2, 4, 6, 1, 16), ('generic', 1, 6, 4, 4, 16),
        ('generic', 1, 6, 4, 4, 20), ('generic', 1, 4, 6, 16, 64), ('generic', 1, 2, 2, 16, 80), ('generic', 1, 260, 260, 4, 16)]
# k / 256 and 2 k / 256 - 1 have at most 8 significant bits - bf16 numbers; (k + 128) / 512 has 9 where k + 128 >= 256 is odd: an exact
# tie, of both parities.  So only (1/2, 1/4) rounds, and the cases above the grid cap use it.
AFFINE_CASES = [dict(route=r, n=n, h=h, w=w, c=c, cp=cp, ab=(2 if h > 100 else i % 3)) for i, (r, n, h, w, c, cp) in enumerate(_AFF)] + \
               [dict(route='affine3', n=1, h=6, w=10, c=3, cp=16, ab=k) for k in (0, 2)] + \
               [dict(route='generic', n=1, h=6, w=4, c=4, cp=20, ab=k) for k in (0, 1)]
for _c in AFFINE_CASES:
    _items = _c['n'] * (_c['h'] // 2) * (_c['w'] // 2) * (1 if _c['route'] == 'affine3' else _c['cp'])
    _c['name'] = 's2d2-{route}-{n}x{h}x{w}x{c}-cp{cp}-ab{ab}'.format(**_c) + ('-second-trip' if _items > LCAP else '')


def affine_route(c, cp):
    return 'affine3' if (c == 3 and cp == 16) else 'generic'


def affine_reference(x, cp, a, b, bug=None):
    """y[by][bx][(2 pr + pc) c + ci] = bf16(a x[2 by + pr][2 bx + pc][ci] + b), block channels >= 4 c are +0.0; -> uint16 bits.
    With pixels k / 256 and the (a, b) of AFFINE_AB the fused multiply-add is exact (asserted), so there is one rounding."""
    n, h, w, c = x.shape
    v = np.float64(F32(a)) * x.astype(np.float64) + np.float64(F32(b))
    assert np.array_equal(v.astype(F32).astype(np.float64), v), 'a x + b is not a float32 number'
    bits = bf16_bits(v.astype(F32), truncate=(bug == 'trunc'))
    y = np.full((n, h // 2, w // 2, cp), 0xa5a5 if bug == 'pad' else 0, np.uint16)
    for pr in range(2):
        for pc in range(2):
            ph = (2 * pc + pr) if bug == 'swap' else (2 * pr + pc)
            y[..., ph * c:(ph + 1) * c] = bits[:, pr::2, pc::2, :]
    return y


def affine_case(c):
    assert affine_route(c['c'], c['cp']) == c['route']
    rng = np.random.default_rng(_seed('affine', c['n'], c['h'], c['w'], c['c']))
    x = (rng.integers(0, 257, size=(c['n'], c['h'], c['w'], c['c'])) / 256.0).astype(F32)
    a, b = AFFINE_AB[c['ab']]
    ref = affine_reference(x, c['cp'], a, b)
    if x.size >= 48 and c['ab'] == 2:
        assert not np.array_equal(ref, affine_reference(x, c['cp'], a, b, bug='trunc')), 'no value rounds up: truncation would pass'
    assert_no_denormals(x, what=c['name'])
    assert_all_written(ref, c['name'])
    return dict(x=x, a=a, b=b, ref=ref)


# ----------------------------------------------------------------------------------------------------------------------
# 5. data feed (csrc/datafeed.hip)
def stats_exact(rgb_image, xx, yy, p):
    """(S, SS, n) of the patch as Python integers."""
    patch = rgb_image[yy:yy + p, xx:xx + p].astype(np.int64)
    assert patch.shape == (p, p, 3)
    return int(patch.sum()), int((patch * patch).sum()), 3 * p * p


def stats_reference(rgb_image, xx, yy, p):
    """-> (mean as a float - the ONE correctly rounded division the kernel does, exact variance as a Fraction)."""
    S, SS, n = stats_exact(rgb_image, xx, yy, p)
    assert n * SS - S * S >= 0 and n * SS < 2 ** 64
    return float(Fraction(S, 255 * n)), Fraction(n * SS - S * S, n * n * 65025)


VAR_BOUND = Fraction(4, 2 ** 53)       # three roundings (numerator, denominator, quotient): (1 + u)^3 - 1 < 4 u, u = 2^-53


def assert_stats(var, mean, rgb_image, xx, yy, p, what=''):
    m, v = stats_reference(rgb_image, xx, yy, p)
    assert float(mean) == m, '{}: mean {!r} != {!r}'.format(what, float(mean), m)
    assert abs(Fraction(float(var)) - v) <= VAR_BOUND * v, '{}: var {!r} outside 4 * 2^-53 of {!r}'.format(what, float(var), float(v))
    if v == 0:
        assert float(var) == 0.0


def _noise_images(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 3)).astype(np.uint8)


def _big_images():
    """1024 x 1024: all-255 (the largest S and SS), a 0 / 255 checkerboard over (y + x + channel) (variance exactly 1/4), noise."""
    img = np.zeros((3, 1024, 1024, 3), np.uint8)
    img[0] = 255
    yy, xx, cc = np.meshgrid(np.arange(1024), np.arange(1024), np.arange(3), indexing='ij')
    img[1] = np.where((yy + xx + cc) % 2 == 0, 0, 255)
    img[2] = _noise_images(1, 1024, 1024, 77)[0]
    return img


def _corner_cands(h, w, p, b, attempts, seed):
    """(b, attempts, 2) even corners: (0, 0) first, (w - p, h - p) last, random even positions between."""
    rng = np.random.default_rng(seed)
    cand = np.stack([2 * (rng.integers(0, w - p + 1, (b, attempts)) // 2), 2 * (rng.integers(0, h - p + 1, (b, attempts)) // 2)], axis=2)
    cand[0, 0] = (0, 0)
    cand[-1, -1] = (w - p, h - p)
    return cand.astype(np.int32)


STATS_CASES = [dict(name='stats-p2-under-one-wave', images='small', p=2, b=3, attempts=4),
               dict(name='stats-p10-under-256-items', images='small', p=10, b=3, attempts=4),
               dict(name='stats-p14-second-loop-trip', images='small', p=14, b=3, attempts=4),
               dict(name='stats-p96-w130', images='small', p=96, b=3, attempts=4),
               dict(name='stats-p96-w-equals-p', images='square96', p=96, b=2, attempts=1),
               dict(name='stats-p1024-extremes', images='big', p=1024, b=3, attempts=1),
               dict(name='stats-one-candidate', images='small', p=10, b=1, attempts=1),
               dict(name='stats-4096-candidates', images='small', p=2, b=64, attempts=64)]


def stats_case(c, cache={}):
    """-> dict(rgb (n, h, w, 3) uint8, image_idx (b), cand (b, attempts, 2)); the last batch entry is the last image."""
    kind = c['images']
    if kind not in cache:
        if kind == 'small':
            img = _noise_images(6, 96, 130, 5)
            img[4] = 200                                           # exactly flat
            img[5, :, :, :] = (np.arange(130)[None, :, None] * 2 % 256).astype(np.uint8)
        elif kind == 'square96':
            img = _noise_images(2, 96, 96, 6)
        else:
            img = _big_images()
        img.setflags(write=False)
        cache[kind] = img
    rgb = cache[kind]
    n, h, w, _ = rgb.shape
    b, attempts, p = c['b'], c['attempts'], c['p']
    idx = (np.arange(b) % n).astype(np.int32)
    idx[-1] = n - 1
    if kind == 'big':
        idx = np.arange(3, dtype=np.int32)
    if kind == 'small' and b >= 3:
        idx[1] = 4
    cand = _corner_cands(h, w, p, b, attempts, _seed('cand', p, b, attempts))
    assert cand.min() >= 0 and (cand[..., 0] + p <= w).all() and (cand[..., 1] + p <= h).all() and not (cand & 1).any()
    if b * attempts > 1 or w == p:
        assert tuple(cand[0, 0]) == (0, 0)
    if b * attempts > 1:
        assert tuple(cand[-1, -1]) == (w - p, h - p) and idx[-1] == n - 1
    return dict(rgb=rgb, image_idx=idx, cand=cand)


# ---- the sampling policy on designed statistics
F_, M_, T_ = 0.001, 0.007, 0.5           # flat (< 0.005), mid (0.005 <= v < 0.01), textured


def _sel(name, mode, var, mean=None, uni=None, max_attempts=3, want=None, branches=()):
    A = len(var)
    return dict(name=name, mode=mode, var=list(var), mean=list(mean) if mean is not None else [0.5] * A,
                uni=list(uni) if uni is not None else [0.0] * A, attempts=A, max_attempts=max_attempts, want=want, branches=tuple(branches))


_OK = (0.001, 0.5)                       # a dark-n-textured patch that is accepted
SELECT_CASES = [
    _sel('none-attempts-1', None, [0.0], want=(0, 1), branches=['none-first-taken']),
    _sel('none-first-taken', None, [0.0] * 6, want=(0, 1), branches=['none-first-taken']),
    _sel('flat-accept', 'flat', [T_, F_, F_, F_, F_, F_], want=(0, 1), branches=['flat-accept']),
    _sel('flat-v-exactly-0.01-accepts-without-a-coin', 'flat', [0.01, T_, T_, T_, T_, T_], want=(0, 1), branches=['flat-accept']),
    _sel('flat-v-exactly-0.005-is-not-flat', 'flat', [0.005, F_, F_, F_, T_, T_], uni=[0.25] * 6, want=(3, 4),
         branches=['flat-coin-lost', 'flat-panic-exhausted']),
    _sel('flat-coin-won', 'flat', [M_, F_, F_, F_, F_, F_], uni=[0.75] * 6, want=(0, 1), branches=['flat-coin-won']),
    _sel('flat-coin-lost', 'flat', [M_, T_, F_, F_, F_, F_], uni=[0.25] * 6, want=(1, 2), branches=['flat-coin-lost', 'flat-accept']),
    _sel('flat-coin-exactly-half-is-lost', 'flat', [M_, T_, F_, F_, F_, F_], uni=[0.5] * 6, want=(1, 2), branches=['flat-coin-half']),
    _sel('flat-panic-takes-the-current', 'flat', [F_, F_, F_, T_, T_, T_], want=(2, 3), branches=['flat-panic-exhausted']),
    _sel('flat-max-attempts-1', 'flat', [F_, T_, T_, T_, T_, T_], max_attempts=1, want=(0, 1), branches=['flat-panic-exhausted']),
    _sel('flat-max-attempts-above-attempts', 'flat', [F_, F_, F_], max_attempts=5, want=(2, 3), branches=['list-runs-out']),
    _sel('flat-list-runs-out', 'flat', [M_] * 6, uni=[0.25, 0.5, 0.0, 0.125, 0.375, 0.4375], want=(5, 6), branches=['list-runs-out']),
    _sel('flat-attempts-1', 'flat', [M_], uni=[0.25], want=(0, 1), branches=['list-runs-out']),
    _sel('aggr-accept-after-flats', 'flat-aggressive', [0.001, 0.015, T_, T_, T_, T_], want=(2, 3), branches=['aggr-accept']),
    _sel('aggr-v-exactly-0.02-accepts', 'flat-aggressive', [0.001, 0.02, T_, T_, T_, T_], want=(1, 2), branches=['aggr-accept']),
    _sel('aggr-best-is-the-first', 'flat-aggressive', [0.015, 0.001, 0.002, T_, T_, T_], want=(0, 3), branches=['aggr-panic-best']),
    _sel('aggr-best-replaced-by-a-later-larger', 'flat-aggressive', [0.001, 0.015, 0.002, T_, T_, T_], want=(1, 3),
         branches=['aggr-best-replaced', 'aggr-panic-best']),
    _sel('aggr-best-replaced-at-the-panic', 'flat-aggressive', [0.001, 0.002, 0.015, T_, T_, T_], want=(2, 3), branches=['aggr-best-replaced']),
    _sel('aggr-equal-variance-keeps-the-earlier', 'flat-aggressive', [0.01, 0.01, 0.001, T_, T_, T_], want=(0, 3), branches=['aggr-best-kept-on-equal']),
    _sel('aggr-max-attempts-1', 'flat-aggressive', [0.001, T_, T_], max_attempts=1, want=(0, 1), branches=['aggr-panic-best']),
    _sel('aggr-list-runs-out', 'flat-aggressive', [0.001, 0.015], max_attempts=5, want=(1, 2), branches=['list-runs-out']),
    _sel('dnt-accept', 'dark-n-textured', [_OK[0]] * 6, [_OK[1]] * 6, want=(0, 1), branches=['dnt-accept']),
    _sel('dnt-reject-v-exactly-0', 'dark-n-textured', [0.0, _OK[0]], [0.5, _OK[1]], want=(1, 2), branches=['dnt-reject-v-zero']),
    _sel('dnt-reject-v-exactly-0.005', 'dark-n-textured', [0.005, _OK[0]], [0.5, _OK[1]], want=(1, 2), branches=['dnt-reject-v-high']),
    _sel('dnt-reject-v-above', 'dark-n-textured', [0.1, _OK[0]], [0.5, _OK[1]], want=(1, 2), branches=['dnt-reject-v-high']),
    _sel('dnt-reject-m-exactly-0.35', 'dark-n-textured', [0.001, _OK[0]], [0.35, _OK[1]], want=(1, 2), branches=['dnt-reject-m-low']),
    _sel('dnt-reject-m-below', 'dark-n-textured', [0.001, _OK[0]], [0.1, _OK[1]], want=(1, 2), branches=['dnt-reject-m-low']),
    _sel('dnt-reject-m-exactly-0.99', 'dark-n-textured', [0.001, _OK[0]], [0.99, _OK[1]], want=(1, 2), branches=['dnt-reject-m-high']),
    _sel('dnt-reject-m-above', 'dark-n-textured', [0.001, _OK[0]], [0.995, _OK[1]], want=(1, 2), branches=['dnt-reject-m-high']),
    _sel('dnt-best-updated-when-both-hold', 'dark-n-textured', [0.1, 0.15, 0.5, _OK[0]], [0.2, 0.3, 0.1, _OK[1]], want=(1, 3),
         branches=['dnt-best-updated', 'dnt-panic-best']),
    _sel('dnt-best-kept-when-only-the-variance-holds', 'dark-n-textured', [0.1, 0.15, 0.5, _OK[0]], [0.2, 0.21, 0.1, _OK[1]], want=(0, 3),
         branches=['dnt-best-kept-var-only', 'dnt-panic-best']),
    _sel('dnt-best-kept-when-only-the-mean-holds', 'dark-n-textured', [0.1, 0.3, 0.5, _OK[0]], [0.2, 0.5, 0.1, _OK[1]], want=(0, 3),
         branches=['dnt-best-kept-mean-only', 'dnt-panic-best']),
    _sel('dnt-best-updated-at-the-panic', 'dark-n-textured', [0.1, 0.5, 0.15, _OK[0]], [0.2, 0.1, 0.3, _OK[1]], want=(2, 3),
         branches=['dnt-best-updated']),
    _sel('dnt-max-attempts-1', 'dark-n-textured', [0.0, _OK[0]], [0.5, _OK[1]], max_attempts=1, want=(0, 1), branches=['dnt-panic-best']),
    _sel('dnt-list-runs-out', 'dark-n-textured', [0.1, 0.15], [0.2, 0.3], max_attempts=5, want=(1, 2), branches=['list-runs-out']),
]
SELECT_BRANCHES = ['none-first-taken', 'flat-accept', 'flat-coin-won', 'flat-coin-lost', 'flat-coin-half', 'flat-panic-exhausted',
                   'list-runs-out', 'aggr-accept', 'aggr-best-replaced', 'aggr-best-kept-on-equal', 'aggr-panic-best', 'dnt-accept',
                   'dnt-reject-v-zero', 'dnt-reject-v-high', 'dnt-reject-m-low', 'dnt-reject-m-high', 'dnt-best-updated',
                   'dnt-best-kept-var-only', 'dnt-best-kept-mean-only', 'dnt-panic-best']
SELECT_BATCH_SIZES = [1, 64, 65, 130]


def select_reference(case, policy=odf.Policy):
    """The policy walked over the case's designed statistics exactly as oracle.datafeed.select walks it over an image: ->
    ((index of the candidate taken, candidates consumed), the set of branches the walk went through).  The branches are read off
    the POLICY's state and answers (panic, best, found), not off the kernel."""
    pol = policy(case['mode'], case['max_attempts'])
    seen = set()
    uni = [float(F32(u)) for u in case['uni']]
    for k in range(case['attempts']):
        v, m = case['var'][k], case['mean'][k]
        coin = []
        best0, panic0 = pol.best, pol.panic
        found, at = pol.step(k, v, m, lambda: coin.append(uni[k]) or uni[k])
        d = case['mode']
        if not d:
            seen.add('none-first-taken')
        elif d == 'flat':
            if coin:
                seen.add('flat-coin-half' if uni[k] == 0.5 else ('flat-coin-won' if found else 'flat-coin-lost'))
            elif pol.panic < panic0:
                if found:
                    seen.add('flat-panic-exhausted')
            else:
                seen.add('flat-accept')
        elif d == 'flat-aggressive':
            if pol.panic == panic0:
                seen.add('aggr-accept')
            else:
                if best0 is not None and pol.best[0] != best0[0]:
                    seen.add('aggr-best-replaced')
                if best0 is not None and pol.best[0] == best0[0] and v == best0[2]:
                    seen.add('aggr-best-kept-on-equal')
                if found:
                    seen.add('aggr-panic-best')
        else:
            if pol.panic == panic0:
                seen.add('dnt-accept')
            else:
                v_ok, m_ok = 0 < v < 0.005, 0.35 < m < 0.99
                if m_ok and not v_ok:
                    seen.add('dnt-reject-v-zero' if v == 0 else 'dnt-reject-v-high')
                if v_ok and not m_ok:
                    seen.add('dnt-reject-m-low' if m <= 0.35 else 'dnt-reject-m-high')
                if best0 is not None:
                    cv, cm = v < 2 * best0[2], m > 1.1 * best0[1]
                    if pol.best[0] != best0[0]:
                        assert cv and cm
                        seen.add('dnt-best-updated')
                    elif cv and not cm:
                        seen.add('dnt-best-kept-var-only')
                    elif cm and not cv:
                        seen.add('dnt-best-kept-mean-only')
                if found:
                    seen.add('dnt-panic-best')
        if found:
            return (at, k + 1), seen
    seen.add('list-runs-out')
    return (case['attempts'] - 1, case['attempts']), seen


class PolicyWithInclusiveBounds(odf.Policy):
    """The wrong policy of the self-test: every strict comparison made inclusive."""

    def step(self, k, var, mean, uniform):
        d = self.discard
        if d == 'flat':
            if var <= 0.005:
                self.panic -= 1
                return (not self.panic > 0), k
            if var <= 0.01:
                return uniform() >= 0.5, k
            return True, k
        if d == 'flat-aggressive':
            if var <= 0.02:
                if self.panic == self.max_attempts or var >= self.best[2]:
                    self.best = (k, mean, var)
                self.panic -= 1
                found = not self.panic > 0
                return found, (self.best[0] if found else k)
            return True, k
        if d == 'dark-n-textured':
            if 0 <= var <= 0.005 and 0.35 <= mean <= 0.99:
                return True, k
            if self.panic == self.max_attempts or (var <= 2 * self.best[2] and mean >= 1.1 * self.best[1]):
                self.best = (k, mean, var)
            self.panic -= 1
            found = not self.panic > 0
            return found, (self.best[0] if found else k)
        return True, k


def select_case(case):
    """-> dict(cand (1, A, 2) int32 with distinct corners, var, mean (float64), uni (float32), want_xy, want_used); asserts on the
    oracle that the case reaches the branches its entry names and gives the answer it was designed for."""
    (at, used), seen = select_reference(case)
    assert (at, used) == case['want'], '{}: the oracle answers {}, the case was designed for {}'.format(case['name'], (at, used), case['want'])
    assert set(case['branches']) <= seen, '{}: reaches {}, not {}'.format(case['name'], sorted(seen), case['branches'])
    A = case['attempts']
    cand = np.stack([2 * np.arange(A) + 10, 100 - 2 * np.arange(A)], axis=1).astype(np.int32)[None]
    return dict(cand=cand, var=np.array([case['var']], np.float64), mean=np.array([case['mean']], np.float64),
                uni=np.array([case['uni']], F32), want_xy=cand[0, at].tolist(), want_used=used, seen=seen)


def select_batch(mode, b):
    """b lanes cycling over the designed cases of `mode` that share attempts = 6 and max_attempts = 3 (padded with accepted
    candidates where a case is shorter - the walk never gets there, asserted); every lane has its own corners."""
    pool = [c for c in SELECT_CASES if c['mode'] == mode and c['max_attempts'] == 3 and c['attempts'] <= 6 and
            'list-runs-out' not in select_reference(c)[1]]
    assert len(pool) >= 2
    var, mean, uni, want = [], [], [], []
    for lane in range(b):
        c = pool[lane % len(pool)]
        pad = 6 - c['attempts']
        var.append(c['var'] + [T_ if mode != 'dark-n-textured' else _OK[0]] * pad)
        mean.append(c['mean'] + [_OK[1]] * pad)
        uni.append(c['uni'] + [0.75] * pad)
        want.append(select_reference(c)[0])
    cand = np.zeros((b, 6, 2), np.int32)
    cand[..., 0] = 2 * (np.arange(b)[:, None] * 6 + np.arange(6)[None, :])
    cand[..., 1] = 4000 - cand[..., 0]
    return dict(cand=cand, var=np.array(var, np.float64), mean=np.array(mean, np.float64), uni=np.array(uni, F32),
                want_xy=[cand[i, w[0]].tolist() for i, w in enumerate(want)], want_used=[w[1] for w in want])


# ---- flat patches in dark-n-textured: the device's exact zero and the oracle's np.var residue, side by side
FLAT_LEVELS = [128, 200, 150]


def flat_patch_case(p=64):
    """Exactly flat images at levels 128, 200 and 150 (means 0.502, 0.784, 0.588: inside (0.35, 0.99)) and one that is flat (200) in
    its upper half and textured below.  np.var(patch / 255) of a flat 64 x 64 x 3 patch is a positive rounding residue at levels
    200 and 150 and exactly 0 at level 128 - 128 / 255 times a power of two is summed without error - (all three asserted here, on the
    CPU).  So at 200 and 150 the ORACLE accepts candidate 0 at once, while the device, whose variance is exactly 0, walks on; at
    128 the two agree.  Candidates of a flat lane: three flat patches; of lane 3: two flat ones, then the textured one."""
    h, w = 2 * p, 2 * p
    rgb = np.zeros((4, h, w, 3), np.uint8)
    rgb[0], rgb[1], rgb[2] = FLAT_LEVELS
    rgb[3, :p] = FLAT_LEVELS[1]
    rgb[3, p:] = np.random.default_rng(3).integers(150, 166, size=(p, w, 3))      # mean ~ 0.62, variance ~ 0.0003
    flat3 = [(0, 0), (2, 2), (4, 4)]
    cand = np.array([flat3, flat3, flat3, [(0, 0), (2, 0), (0, p)]], np.int32)
    idx = np.arange(4, dtype=np.int32)
    positive = []
    for i in range(4):
        for k in range(2):
            v, m = odf.patch_stats(rgb[i], cand[i, k, 0], cand[i, k, 1], p)
            assert 0 <= v < 1e-30 and 0.35 < m < 0.99
            assert stats_reference(rgb[i], cand[i, k, 0], cand[i, k, 1], p)[1] == 0
        positive.append(v > 0)
    assert positive == [False, True, True, True], 'np.var of the flat patches: {}'.format(positive)
    v, m = odf.patch_stats(rgb[3], 0, p, p)
    assert 0 < v < 0.005 and 0.35 < m < 0.99 and stats_reference(rgb[3], 0, p, p)[1] > 0
    oracle = {ma: [odf.select(rgb[i], [tuple(c) for c in cand[i]], [0.0] * 3, p, 'dark-n-textured', ma) for i in range(4)] for ma in (2, 3)}
    # the oracle: level 128 is rejected (var == 0 there too) until the panic counter runs out and the best - the first - is taken;
    # every other lane takes candidate 0 at once
    for ma in (2, 3):
        assert [list(o[0]) for o in oracle[ma]] == [[0, 0]] * 4 and [o[1] for o in oracle[ma]] == [ma, 1, 1, 1]
    # the device: var == 0 is rejected on every flat patch.  max_attempts = 2: every lane panics at candidate 1 and returns its best
    # (candidate 0: candidate 1 has the same mean, not one 1.1 times larger); max_attempts = 3: lanes 0 .. 2 the same one candidate
    # later, lane 3 reaches its textured candidate and accepts it
    device = {2: dict(xy=[[0, 0]] * 4, used=[2, 2, 2, 2]), 3: dict(xy=[[0, 0], [0, 0], [0, 0], [0, p]], used=[3, 3, 3, 3])}
    return dict(rgb=rgb, image_idx=idx, cand=cand, p=p, oracle=oracle, device=device)


# ---- gather
def every_value_images():
    """raw (1, 256, 256, 4): every uint16 value in every plane, under four different permutations; rgb (1, 512, 512, 3): every
    byte in every channel (1024 times, shuffled)."""
    rng = np.random.default_rng(11)
    raw = np.stack([rng.permutation(65536) for _ in range(4)], axis=-1).astype(np.uint16).reshape(1, 256, 256, 4)
    rgb = np.stack([rng.permutation(np.tile(np.arange(256), 1024)) for _ in range(3)], axis=-1).astype(np.uint8).reshape(1, 512, 512, 3)
    for p in range(4):
        assert len(np.unique(raw[..., p])) == 65536
        assert p == 0 or not np.array_equal(raw[..., p], raw[..., 0])
    for ch in range(3):
        assert len(np.unique(rgb[..., ch])) == 256
    return raw, rgb


GATHER_CASES = [dict(name='gather-every-value-cut-whole', images='every', p=512, b=1, kind='both'),
                dict(name='gather-p2-one-raw-pixel-corners', images='small', p=2, b=5, kind='both'),
                dict(name='gather-p10-corners', images='small', p=10, b=5, kind='both'),
                dict(name='gather-rgb-b6-p512-second-trip', images='every', p=512, b=6, kind='rgb'),
                dict(name='gather-raw-b9-p1024-second-trip', images='big', p=1024, b=9, kind='raw')]


def gather_case(c, cache={}):
    kind = c['images']
    if kind not in cache:
        if kind == 'every':
            raw, rgb = every_value_images()
        elif kind == 'small':
            rng = np.random.default_rng(12)
            raw = rng.integers(0, 65536, size=(3, 48, 65, 4)).astype(np.uint16)
            rgb = rng.integers(0, 256, size=(3, 96, 130, 3)).astype(np.uint8)
        else:
            raw = np.random.default_rng(13).integers(0, 65536, size=(2, 512, 512, 4)).astype(np.uint16)
            rgb = None
        cache[kind] = (raw, rgb)
    raw, rgb = cache[kind]
    n, h, w = raw.shape[0], 2 * raw.shape[1], 2 * raw.shape[2]
    p, b = c['p'], c['b']
    idx = (np.arange(b) % n).astype(np.int32)
    idx[-1] = n - 1
    xy = _corner_cands(h, w, p, b, 1, _seed('gather', p, b))[:, 0, :]
    if b > 1:
        assert tuple(xy[0]) == (0, 0) and tuple(xy[-1]) == (w - p, h - p)
    want_raw, want_rgb = c['kind'] in ('both', 'raw'), c['kind'] in ('both', 'rgb')
    x, y = odf.cut_batch(raw if want_raw else None, rgb if want_rgb else None, idx, [tuple(v) for v in xy], p)
    if want_raw:
        assert b * (p // 2) ** 2 > GCAP or 'second-trip' not in c['name']
    else:
        assert b * p * (3 * p // 2) > GCAP or 'second-trip' not in c['name']
    return dict(raw=raw if want_raw else None, rgb=rgb if want_rgb else None, n=n, h=h, w=w, image_idx=idx, xy=xy.astype(np.int32), x=x, y=y)
