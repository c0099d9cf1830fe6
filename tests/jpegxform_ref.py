"""Plain numpy restatement of the lossless transforms over jpegrst_ref.py, jpegsamp_ref.py, jpegdprog_ref.py and
jpeggrey_ref.py: what a flip, a transposition, a rotation and an aligned crop do to the quantised coefficients and the quantisation tables
of a file, the geometry of the file that results, the two edge rules - and transcode(), which reads a file with the reference readers,
transforms it and writes it with the reference writers.  Test infrastructure - the product never imports it.

A block is C[v][u], v vertical.  Mirroring left to right reverses the block columns of every component and negates odd u, top to bottom
the block rows and odd v, transposing swaps block rows with columns and C[v][u] with C[u][v] (and transposes every table).  Here each
operation is carried out step by step, as the composition it is named after - the product does each as one gather."""
import numpy as np

import jpeg_ref as ref
import jpegdprog_ref as dprog
import jpeggrey_ref as grey
import jpegprog_ref as pref
import jpegrst_ref as rst

OPS = ('none', 'hflip', 'vflip', 'transpose', 'transverse', 'rot90', 'rot180', 'rot270')       # jpegtran's names, the ABI's order
# every operation as a sequence of the three elementary ones
STEPS = {'none': (), 'hflip': ('hflip',), 'vflip': ('vflip',), 'transpose': ('transpose',), 'rot90': ('transpose', 'hflip'),
         'rot270': ('transpose', 'vflip'), 'rot180': ('hflip', 'vflip'), 'transverse': ('transpose', 'hflip', 'vflip')}
INVERSE = {'none': 'none', 'hflip': 'hflip', 'vflip': 'vflip', 'transpose': 'transpose', 'transverse': 'transverse', 'rot90': 'rot270',
           'rot180': 'rot180', 'rot270': 'rot90'}
TRANSPOSING = ('transpose', 'transverse', 'rot90', 'rot270')
# (the width, the height) must be a whole number of source iMCUs
WHOLE = {'none': (False, False), 'transpose': (False, False), 'hflip': (True, False), 'rot270': (True, False), 'vflip': (False, True),
         'rot90': (False, True), 'rot180': (True, True), 'transverse': (True, True)}
GREY = (0, 0)


def pixels(img, op):
    """The geometric operation itself on an array (rows, cols, ...): what the decoded image of the output file looks like."""
    for step in STEPS[op]:
        img = {'hflip': lambda a: a[:, ::-1], 'vflip': lambda a: a[::-1], 'transpose': lambda a: np.swapaxes(a, 0, 1)}[step](img)
    return img


def _negate(c):
    return (-c.astype(np.int32)).astype(np.int16)               # two's complement on 16 bits: -(-32768) stays -32768


def _step(comp, step):
    """One component (block rows, block cols, 64 zig-zag) int16 through one elementary operation."""
    nat = np.zeros(comp.shape, np.int16)
    nat[..., ref.ZZ] = comp
    nat = nat.reshape(comp.shape[:2] + (8, 8))                  # [block row][block col][v][u]
    if step == 'hflip':
        nat = nat[:, ::-1].copy()
        nat[..., 1::2] = _negate(nat[..., 1::2])
    elif step == 'vflip':
        nat = nat[::-1].copy()
        nat[..., 1::2, :] = _negate(nat[..., 1::2, :])
    else:
        nat = nat.transpose(1, 0, 3, 2)
    return np.ascontiguousarray(nat.reshape(nat.shape[:2] + (64,))[..., ref.ZZ])


def component(comp, op):
    for step in STEPS[op]:
        comp = _step(comp, step)
    return comp


def tables(qt, op):
    """(T, 64) tables in natural order: every one transposed by the transposing operations."""
    qt = np.asarray(qt)
    return qt.reshape(-1, 8, 8).transpose(0, 2, 1).reshape(-1, 64).copy() if op in TRANSPOSING else qt.copy()


def imcu(hs, vs):
    """(rows, cols) of the iMCU; 8 x 8 in a grey-scale file whatever it declares."""
    return (8, 8) if (hs, vs) == GREY else (8 * vs, 8 * hs)


def region(h, w, hs, vs, op, crop=None, edge='perfect'):
    """(x, y, width, height) of the source that the operation moves: the crop, trimmed; every refusal a ValueError."""
    if op not in OPS or edge not in ('perfect', 'trim'):
        raise ValueError('unknown operation or edge rule')
    mh, mw = imcu(hs, vs)
    x, y, cw, ch = (0, 0, w, h) if crop is None else crop
    if cw < 1 or ch < 1 or x < 0 or y < 0 or x + cw > w or y + ch > h:
        raise ValueError('crop outside the image')
    if x % mw or y % mh:
        raise ValueError('crop origin not aligned: below it {} {}'.format(x - x % mw, y - y % mh))
    if WHOLE[op][0] and cw % mw:
        if edge == 'perfect':
            raise ValueError('partial iMCU: width')
        cw -= cw % mw
    if WHOLE[op][1] and ch % mh:
        if edge == 'perfect':
            raise ValueError('partial iMCU: height')
        ch -= ch % mh
    if cw < 1 or ch < 1:
        raise ValueError('nothing left')
    return x, y, cw, ch


def size(h, w, hs, vs, op, crop=None, edge='perfect'):
    """(h', w', hs', vs')"""
    _, _, cw, ch = region(h, w, hs, vs, op, crop, edge)
    return (cw, ch, vs, hs) if op in TRANSPOSING else (ch, cw, hs, vs)


def shapes(h, w, hs, vs):
    """[(block rows, block cols)] of the real blocks per component."""
    if (hs, vs) == GREY:
        return [grey.geometry(h, w)]
    return [(c[2], c[3]) for c in ref.geometry(h, w, hs, vs)[0]]


def transform(coefs, h, w, hs, vs, op, crop=None, edge='perfect'):
    """[component (block rows, block cols, 64)] of an h x w file -> (the components of the output file, h', w', hs', vs').  The region is
    cut out block-wise - the chroma origin is (x / hs, y / vs) samples - and the blocks at a new edge keep their contents."""
    x, y, cw, ch = region(h, w, hs, vs, op, crop, edge)
    mh, mw = imcu(hs, vs)
    out = []
    for k, (comp, (rows, cols)) in enumerate(zip(coefs, shapes(ch, cw, hs, vs))):
        r0, c0 = (y // 8, x // 8) if k == 0 else (y // mh, x // mw)
        part = comp[r0:r0 + rows, c0:c0 + cols]
        assert part.shape[:2] == (rows, cols)
        out.append(component(part, op))
    return (out,) + size(h, w, hs, vs, op, crop, edge)


def flat(coefs):
    return np.concatenate([np.asarray(c, np.int16).reshape(-1) for c in coefs])


def unflat(vector, h, w, hs, vs):
    out, at = [], 0
    for rows, cols in shapes(h, w, hs, vs):
        out.append(np.asarray(vector[at:at + rows * cols * 64], np.int16).reshape(rows, cols, 64))
        at += rows * cols * 64
    assert at == len(vector)
    return out


# ---- files ----------------------------------------------------------------------------------------------------------------------------
def _sof(data):
    """(marker, components) of the frame header."""
    i = 2
    while True:
        marker, length = data[i + 1], int.from_bytes(data[i + 2:i + 4], 'big')
        if marker in (0xc0, 0xc2):
            return marker, data[i + 4 + 5]
        i += 2 + length


def parse(data):
    """A file of the kinds the product reads -> dict(h, w, hs, vs - GREY for one component -, ri, qtables (3 | 1, 64) per component in
    natural order, coefs [component (block rows, block cols, 64) int16])."""
    marker, ncomp = _sof(data)
    if ncomp == 1:
        p = grey.split(data)
        h, w = p['h'], p['w']
        coef = grey.decode_progressive(data)[0] if p['progressive'] else grey.decode_baseline(data)
        return dict(h=h, w=w, hs=0, vs=0, ri=p['ri'], qtables=np.asarray(p['qtable'], np.int64).reshape(1, 64),
                    coefs=[np.asarray(coef, np.int16).reshape(grey.geometry(h, w) + (64,))])
    if marker == 0xc0:
        p = rst.parse(data)
        return dict(h=p['h'], w=p['w'], hs=p['hs'], vs=p['vs'], ri=p['ri'], qtables=p['qtables'], coefs=p['coefs'])
    p = dprog.split(data)
    vector, status, _ = dprog.decode(data)
    assert status == 0
    return dict(h=p['h'], w=p['w'], hs=p['hs'], vs=p['vs'], ri=p['ri'], qtables=np.stack([p['qtables'][t] for t in p['q']]),
                coefs=unflat(vector, p['h'], p['w'], p['hs'], p['vs']))


def write(coefs, h, w, hs, vs, qtables, ri=0, optimize=True, progressive=False):
    """The file the product writes for these coefficients: JFIF APP0, two DQT segments where the Cb and Cr tables are equal, else three
    (one for a grey-scale file), Annex K's or the optimal Huffman tables, or libjpeg's simple progression."""
    qt = np.asarray(qtables, np.int64)
    if (hs, vs) == GREY:
        assert not progressive
        return grey.encode(coefs[0], h, w, qt[0], ri, optimize)[0]
    qt = qt[:2] if np.array_equal(qt[1], qt[2]) else qt
    if progressive:
        return dprog.encode(coefs, h, w, hs, vs, pref.prefix_of(rst.header(h, w, qt, hs, vs, 0)), dprog.STANDARD, ri)
    return rst.encode(coefs, h, w, qt, hs, vs, ri, optimize)[0]


def transcode(data, op='none', crop=None, edge='perfect', optimize=True, progressive=False):
    """transcode_batch(data, lossless=op, ...) restated: the bytes of the output file."""
    p = parse(data)
    coefs, h, w, hs, vs = transform(p['coefs'], p['h'], p['w'], p['hs'], p['vs'], op, crop, edge)
    return write(coefs, h, w, hs, vs, tables(p['qtables'], op), p['ri'], optimize, progressive)


# ---- the derivation's yardstick: a float inverse DCT ----------------------------------------------------------------------------------
def float_plane(comp, qtable):
    """One component's coefficients, dequantised, through an orthonormal float64 inverse DCT -> its sample plane (8 rows, 8 cols a block),
    without libjpeg's rounding."""
    k = np.arange(8)
    basis = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k[:, None] == 0, np.sqrt(1 / 8), np.sqrt(2 / 8))   # [u][x]
    nat = np.zeros(comp.shape, np.float64)
    nat[..., ref.ZZ] = comp.astype(np.float64)
    blocks = (nat * np.asarray(qtable, np.float64)).reshape(comp.shape[:2] + (8, 8))
    samples = np.einsum('vy,rcvu,ux->rcyx', basis, blocks, basis)
    return samples.transpose(0, 2, 1, 3).reshape(comp.shape[0] * 8, comp.shape[1] * 8)
