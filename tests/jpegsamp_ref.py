"""Plain numpy restatement of how libjpeg reads colour files of any luma sampling over 1x1 chroma over jpeg_ref.py,
jpegscale_ref.py and jpegdprog_ref.py: the geometry for any (hs, vs), the two up-samplers the samplings 1x2, 4x1, 4x2, 1x4 and 2x4 add
(jdsample.c's h1v2 triangle filter and int_upsample's replication) and the rule that picks an up-sampler at every scale.  And a writer of
such files for the tests - box down-sampling, (sum + n / 2) / n, which no libjpeg writer on this machine could be held against: the
files are valid, what they decode to is Pillow's to say (tests/golden/make_jpegsamp_golden.py).  Test infrastructure - the product never
imports it.  All integer arithmetic."""
import numpy as np

import jpeg_ref as ref
import jpegdprog_ref as dprog
import jpegprog_ref as pref
import jpegrst_ref as rst
import jpegscale_ref as sref

THREE = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}
WIDE = {'4:4:0': (1, 2), '4:1:1': (4, 1), '4:1:0': (4, 2), '1x4': (1, 4), '2x4': (2, 4)}
SAMPLINGS = dict(THREE, **WIDE)
SCALES = sref.SCALES


# ---- the writer ---------------------------------------------------------------------------------------------------------------------
def component_planes(rgb, hs, vs):
    """uint8 (H, W, 3) -> the three sample planes over whole MCUs: edges replicated, chroma box down-sampled by (vs, hs)."""
    h, w, _ = rgb.shape
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    hp, wp = -(-h // (8 * vs)) * 8 * vs, -(-w // (8 * hs)) * 8 * hs
    out = []
    for k, p in enumerate((y, cb, cr)):
        p = np.pad(p, ((0, hp - h), (0, wp - w)), mode='edge')
        if k:
            n = hs * vs
            p = (p.reshape(hp // vs, vs, wp // hs, hs).sum(axis=(1, 3)) + n // 2) // n
        out.append(p)
    return out


def coefficients(rgb, quality, hs, vs):
    """uint8 (H, W, 3) -> [Y, Cb, Cr] quantised coefficients (block rows, block cols, 64 zig-zag) of the REAL blocks."""
    comps, _ = ref.geometry(rgb.shape[0], rgb.shape[1], hs, vs)
    out = []
    for k, p in enumerate(component_planes(rgb, hs, vs)):
        bh, bw = p.shape[0] // 8, p.shape[1] // 8
        x = ref.fdct(p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)).reshape(bh, bw, 64)
        qv = ref.qtable(quality, min(k, 1)) << 3
        c = np.sign(x) * ((np.abs(x) + (qv >> 1)) // qv)
        out.append(c[:comps[k][2], :comps[k][3]][..., ref.ZZ].astype(np.int16))
    return out


def qtables(quality):
    return [ref.qtable(quality, 0), ref.qtable(quality, 1), ref.qtable(quality, 1)]


def write_baseline(coefs, h, w, quality, hs, vs, ri=0, optimize=False):
    """The baseline file of the coefficients: jpegrst_ref's writer, which is general in (hs, vs) - Annex K's tables or the optimal ones."""
    return rst.encode(coefs, h, w, rst.quality_tables(quality), hs, vs, ri, optimize)[0]


def write_progressive(coefs, h, w, quality, hs, vs, script, ri=0):
    """The progressive file of `script` (jpegdprog_ref's writer; dprog.STANDARD is libjpeg's simple progression)."""
    prefix = pref.prefix_of(rst.header(h, w, rst.quality_tables(quality), hs, vs, 0))
    return dprog.encode(coefs, h, w, hs, vs, prefix, script, ri)


# ---- the geometry -------------------------------------------------------------------------------------------------------------------
def geometry(h, w, hs, vs):
    """What csrc/jpeg_geo.h's make_geo derives: dict(per, ny, SB, my, mx, bhY, bwY, bhC, bwC, ceh, cew, nbY, nbC, NB)."""
    comps, (my, mx) = ref.geometry(h, w, hs, vs)
    (_, _, bhY, bwY), (_, _, bhC, bwC) = comps[0], comps[1]
    return dict(per=hs * vs + 2, ny=hs * vs, SB=my * mx * (hs * vs + 2), my=my, mx=mx, bhY=bhY, bwY=bwY, bhC=bhC, bwC=bwC,
                ceh=-(-h // vs), cew=-(-w // hs), nbY=bhY * bwY, nbC=bhC * bwC, NB=bhY * bwY + 2 * bhC * bwC)


def upsampler(rx, ry, fancy, cols):
    """jdsample.c's choice for a component whose plane the output exceeds by (rx, ry), by the first rule that applies."""
    if (rx, ry) == (1, 1):
        return 'none'
    if (rx, ry) == (2, 1):
        return 'h2v1' if fancy and cols > 2 else 'replicate'
    if (rx, ry) == (1, 2) and fancy:
        return 'h1v2'
    if (rx, ry) == (2, 2):
        return 'h2v2' if fancy and cols > 2 else 'replicate'
    return 'replicate'


def scaled_geometry(h, w, hs, vs, s):
    """At scale 1 / s (1 included): dict(nY, nC, ehC, ewC, rx, ry, mode, oh, ow) - the block sides, the chroma plane's extent, the
    ratios of the output to it and the up-sampler."""
    m = 8 // s
    nY, nC = sref.block_size(s, hs, vs, hs, vs), sref.block_size(s, 1, 1, hs, vs)
    ehC, ewC = -(-h * nC // (8 * vs)), -(-w * nC // (8 * hs))
    rx, ry = hs * m // nC, vs * m // nC
    assert nY == m and rx * nC == hs * m and ry * nC == vs * m
    return dict(nY=nY, nC=nC, ehC=ehC, ewC=ewC, rx=rx, ry=ry, mode=upsampler(rx, ry, m > 1, ewC), oh=-(-h // s), ow=-(-w // s))


# ---- the decoder --------------------------------------------------------------------------------------------------------------------
def h1v2(p):
    """Rows 2j and 2j + 1 are (3 p[j] + p[j - 1] + 1) >> 2 and (3 p[j] + p[j + 1] + 2) >> 2; the edge row is its own neighbour."""
    up, dn = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
    out = np.empty((2 * p.shape[0], p.shape[1]), np.int64)
    out[0::2], out[1::2] = (3 * p + up + 1) >> 2, (3 * p + dn + 2) >> 2
    return out


def planes(coefs, qt, h, w, hs, vs, s=1):
    """The three sample planes at the output's size, chroma brought up as libjpeg chooses."""
    sg = scaled_geometry(h, w, hs, vs, s)
    out = []
    for k, (c, q) in enumerate(zip(coefs, qt)):
        n = sg['nC'] if k else sg['nY']
        rows, cols = (sg['ehC'], sg['ewC']) if k else (sg['oh'], sg['ow'])
        bh, bw, _ = c.shape
        nat = np.zeros((bh, bw, 64), np.int64)
        nat[..., ref.ZZ] = c.astype(np.int64)
        x = sref.idct_reduced((nat * np.asarray(q, np.int64)).reshape(bh, bw, 8, 8), n)
        p = x.transpose(0, 2, 1, 3).reshape(bh * n, bw * n)[:rows, :cols].astype(np.int64)
        mode = sg['mode'] if k else 'none'
        if mode == 'h2v1':
            p = sref._fancy_h2v1(p)
        elif mode == 'h1v2':
            p = h1v2(p)
        elif mode == 'h2v2':
            p = ref._upsample(p, 2, 2, rows, cols)
        elif mode == 'replicate':
            p = np.repeat(np.repeat(p, sg['ry'], axis=0), sg['rx'], axis=1)
        out.append(p[:sg['oh'], :sg['ow']])
        assert out[-1].shape == (sg['oh'], sg['ow'])
    return out


def decode(coefs, qt, h, w, hs, vs, s=1):
    """The uint8 (ceil(h / s), ceil(w / s), 3) image libjpeg decodes at scale 1 / s."""
    y, cb, cr = planes(coefs, qt, h, w, hs, vs, s)
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
