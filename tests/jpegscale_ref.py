"""Plain numpy restatement of libjpeg's scaled decoding (scale_num / scale_denom = 1 / s, s in 1, 2, 4, 8) over
jpeg_ref.py: the block size of every component (jdmaster.c), the reduced inverse DCTs (jidctred.c), the up-sampling libjpeg then chooses
(jdsample.c) and the unchanged colour conversion.  Test infrastructure - the product never imports it.  All integer arithmetic."""
import numpy as np

import jpeg_ref as ref

SCALES = (1, 2, 4, 8)


def scaled_size(h, w, s):
    return -(-h // s), -(-w // s)


def block_size(s, hc, vc, hmax, vmax):
    """The side N of the block the inverse DCT of a component with the factors (hc, vc) writes at scale 1 / s."""
    m = 8 // s
    n = m
    while n < 8 and (hmax * m) % (hc * n * 2) == 0 and (vmax * m) % (vc * n * 2) == 0:
        n *= 2
    return n


def geometry(h, w, hs, vs, s, nc=3):
    """Per component (N, rows, cols of its scaled plane, up-sampling: 'none' | 'replicate' | 'fancy' | 'full') and the output
    (rows, cols).  'full': scale 1, where the chroma takes jpeg_ref's full-size up-sampling, 2:1 one way or both.  A one-component file
    has N = 8 / s whatever factors it declares."""
    out = []
    for hc, vc in ([(hs, vs), (1, 1), (1, 1)] if nc == 3 else [(1, 1)]):
        hmax, vmax = (hs, vs) if nc == 3 else (1, 1)
        n = block_size(s, hc, vc, hmax, vmax)
        rows, cols = -(-h * vc * n // (vmax * 8)), -(-w * hc * n // (hmax * 8))
        up = 'none'
        if s == 1 and hc != hmax:
            up = 'full'
        elif cols != -(-w // s):                         # 4:2:2 chroma: 2:1 horizontally, at every reduced scale; never vertically
            assert rows == -(-h // s)
            up = 'fancy' if s < 8 and cols > 2 else 'replicate'
        out.append((n, rows, cols, up))
    return out, scaled_size(h, w, s)


def _D(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass4(i, n):
    t0 = i[0] << 14
    t2 = 15137 * i[2] - 6270 * i[6]
    a0 = -1730 * i[7] + 11893 * i[5] - 17799 * i[3] + 8697 * i[1]
    a2 = -4176 * i[7] - 4926 * i[5] + 7373 * i[3] + 20995 * i[1]
    return [_D(v, n) for v in (t0 + t2 + a2, t0 - t2 + a0, t0 - t2 - a0, t0 + t2 - a2)]


def _pass2(i, n):
    t10 = i[0] << 15
    t0 = -5906 * i[7] + 6967 * i[5] - 10426 * i[3] + 29692 * i[1]
    return [_D(t10 + t0, n), _D(t10 - t0, n)]


def idct_reduced(d, n):
    """(..., 8, 8) dequantised coefficients -> (..., n, n) samples 0..255: jpeg_idct_4x4, _2x2, _1x1, and jidctint for n = 8."""
    d = d.astype(np.int64)
    if n == 8:
        return ref.idct(d)
    if n == 1:
        return np.clip(_D(d[..., :1, :1], 3) + 128, 0, 255)
    one, first, second = (_pass4, 12, 19) if n == 4 else (_pass2, 13, 20)
    cols = one([d[..., k, :] for k in range(8)], first)            # every column (those the row pass never reads included): n x (..., 8)
    out = [one([row[..., k] for k in range(8)], second) for row in cols]
    return np.clip(np.stack([np.stack(r, -1) for r in out], -2) + 128, 0, 255)


def _fancy_h2v1(p):
    left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
    return out


def planes(coefs, qtables, h, w, hs, vs, s):
    """[component] real-block coefficients (block rows, block cols, 64 in zig-zag order) and a table per component (natural order) ->
    the components' sample planes at the output's size."""
    geo, (oh, ow) = geometry(h, w, hs, vs, s, len(coefs))
    out = []
    for c, q, (n, rows, cols, up) in zip(coefs, qtables, geo):
        bh, bw, _ = c.shape
        nat = np.zeros((bh, bw, 64), np.int64)
        nat[..., ref.ZZ] = c.astype(np.int64)
        x = idct_reduced((nat * np.asarray(q, np.int64)).reshape(bh, bw, 8, 8), n)
        p = x.transpose(0, 2, 1, 3).reshape(bh * n, bw * n)[:rows, :cols]
        if up == 'full':
            p = ref._upsample(p, hs, vs, rows, cols)
        elif up == 'fancy':
            p = _fancy_h2v1(p)
        elif up == 'replicate':
            p = np.repeat(p, 2, axis=1)
        out.append(p[:oh, :ow])
        assert out[-1].shape == (oh, ow)
    return out


def decode_scaled(coefs, qtables, h, w, hs, vs, s):
    """The uint8 image libjpeg decodes at scale 1 / s: (ceil(h / s), ceil(w / s), 3), or (.., .., 1) from one component."""
    p = planes(coefs, qtables, h, w, hs, vs, s)
    if len(p) == 1:
        return p[0].astype(np.uint8)[..., None]
    y, cb, cr = p[0], p[1] - 128, p[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
