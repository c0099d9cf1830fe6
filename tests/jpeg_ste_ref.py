"""Plain numpy restatement of the real-codec training forward (csrc/jpeg_ste.hip) and the cases its tests
share: jpeg_ref.to_bytes -> the coefficients of jpeg_ref / jpegq_ref -> the body of their decode_u8, keeping the (r, g, b) values
BEFORE the final range limit next to the bytes.  From those: y = u8 / 255 in float32 and mask = sum_c ((0 <= pre_c <= 255) << c).
Test infrastructure like jpeg_ref.py - the product never imports it.  Nothing here needs a GPU."""
import functools

import numpy as np

import djpeg_cases as C
import jpeg_ref as ref
import jpegq_cases
import jpegq_ref as qref

QUALITIES = (10, 50, 95)
INPUTS = ('saturated', 'noise')
# (sub-sampling, (n, h, w)): the 4:4:4 strip / task shapes of the differentiable codec's tests, then its sub-sampled shapes
SHAPES = [('4:4:4', C.CASES[k]) for k in C.CASE_IDS] + list(C.SUB_CASES)
SHAPE_IDS = ['{}-{}x{}x{}'.format(s.replace(':', ''), *shape) for s, shape in SHAPES]
# every shape and input at the three qualities, and every shape once with a caller's three distinct tables
CASES = [(s, shape, kind, q) for s, shape in SHAPES for kind in INPUTS for q in QUALITIES] + \
        [(s, shape, 'saturated', 'three') for s, shape in SHAPES]
CASE_IDS = ['{}-{}x{}x{}-{}-{}'.format(s.replace(':', ''), *shape, kind, 'q{}'.format(q) if q != 'three' else q)
            for s, shape, kind, q in CASES]
USER_SHAPE = (2, 256, 256)      # one user-sized shape per sub-sampling, against the device codec only
CLEAR_SHARE = (0.10, 0.45)      # share of clear mask bits every `saturated` case must have


def tables_of(q):
    """(3, 64) int64 tables, natural order: libjpeg's of a quality 1..100, or the caller's set 'three'."""
    if q == 'three':
        return np.asarray(jpegq_cases.tables('three'), np.int64)
    return np.stack([ref.qtable(q, 0), ref.qtable(q, 1), ref.qtable(q, 1)])


def convert(x):
    """The operator's own input conversion: 255 * v in float32, truncated, clamped to 0..255 - with no batch-wide rescaling."""
    return np.clip(np.trunc(np.float32(255) * np.asarray(x, np.float32)), 0, 255).astype(np.uint8)


def decode_pre(coefs, h, w, tables, hs, vs):
    """The body of decode_u8: real-block coefficients -> (r, g, b) int64 (h, w, 3) before the final range limit."""
    planes = []
    for k, c in enumerate(coefs):
        bh, bw, _ = c.shape
        nat = np.zeros((bh, bw, 64), np.int64)
        nat[..., ref.ZZ] = c.astype(np.int64)
        p = ref.idct((nat * tables[k]).reshape(bh, bw, 8, 8)).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        if k:
            p = ref._upsample(p, hs, vs, -(-h // vs), -(-w // hs))
        planes.append(p[:h, :w])
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.stack([r, g, b], -1)


def restate(xb, tables, subsampling):
    """uint8 (n, h, w, 3) and (3, 64) tables -> dict(u8 (n,h,w,3), y float32, mask (n,h,w) uint8, pre int64), read-only."""
    hs, vs = ref.SUBSAMPLING[subsampling]
    n, h, w, _ = xb.shape
    tables = np.asarray(tables, np.int64)
    pre = np.stack([decode_pre(qref.coefficients(xb[i], tables, hs, vs), h, w, tables, hs, vs) for i in range(n)])
    u8 = np.clip(pre, 0, 255).astype(np.uint8)
    keep = (pre >= 0) & (pre <= 255)
    out = dict(u8=u8, y=u8.astype(np.float32) / np.float32(255), pre=pre,
               mask=(keep[..., 0] * 1 + keep[..., 1] * 2 + keep[..., 2] * 4).astype(np.uint8))
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def image(shape, kind):
    x = C.images(shape, kind)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(sub, shape, kind, q):
    """The restatement of one case, computed once and left unchanged.  The input goes through jpeg_ref.to_bytes: the cases' inputs lie
    in [0, 1], where it is the operator's conversion."""
    return restate(ref.to_bytes(image(shape, kind)), tables_of(q), sub)


@functools.lru_cache(maxsize=None)
def reference_unclipped(sub, shape, q):
    """The restatement fed the operator's own conversion of an input with values below 0 and above 1."""
    return restate(convert(image(shape, 'unclipped')), tables_of(q), sub)


def clear_share(mask):
    """Share of clear bits among the three clip bits of every pixel."""
    m = np.asarray(mask)
    return 1.0 - float(np.stack([(m >> c) & 1 for c in range(3)]).mean())
