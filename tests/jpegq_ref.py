"""Plain numpy restatement of the baseline JPEG codec with the caller's quantisation tables: the arithmetic of
jpeg_ref.py with divisors T << 3 in place of qtable(quality) << 3 - coefficients, the header with two or three DQT segments, whole
files (Annex K or optimal Huffman tables), the decode - and the rule that turns float tables into the entries a file can carry.
Test infrastructure like jpeg_ref.py - the product never imports it.  Tables are (T, 64) integers 1..255 in natural order, T = 2
(luma, chroma) or 3 (Y, Cb, Cr)."""
import numpy as np

import jpeg_ref as ref
import jpegopt_ref as oref

ST_RAISED, ST_LOWERED, ST_NONFINITE = 1, 2, 4        # nimg_jpeg_tables_from_float, per table set
HEADER_BYTES = {2: 623, 3: 692}
DHT_OFFSET = {2: 177, 3: 246}


def per_component(tables):
    """(T, 64) -> (3, 64) int64: with two tables Cr takes the chroma table."""
    t = np.asarray(tables, np.int64).reshape(len(tables), 64)
    return t[[0, 1, 1]] if len(t) == 2 else t


def coefficients(rgb, tables, hs, vs):
    """uint8 (H, W, 3) -> [Y, Cb, Cr] quantised coefficients (block rows, block cols, 64 in zig-zag order) of the REAL blocks."""
    comps, _ = ref.geometry(rgb.shape[0], rgb.shape[1], hs, vs)
    t3 = per_component(tables)
    out = []
    for k, p in enumerate(ref.component_planes(rgb, hs, vs)):
        bh, bw = p.shape[0] // 8, p.shape[1] // 8
        x = ref.fdct(p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)).reshape(bh, bw, 64)
        qv = t3[k] << 3
        c = np.sign(x) * ((np.abs(x) + (qv >> 1)) // qv)
        out.append(c[:comps[k][2], :comps[k][3]][..., ref.ZZ].astype(np.int16))
    return out


def header(h, w, tables, hs, vs, huffman=None):
    """SOI .. SOS: one DQT segment per table, zig-zag; a third table is Cr's (selector 2 in SOF0).  huffman: (4, 272) tables of
    jpegopt_ref in DHT segments of their own, else Annex K's."""
    t = np.asarray(tables, np.int64).reshape(len(tables), 64)
    out = bytes.fromhex('ffd8' 'ffe00010' '4a46494600' '0101' '00' '0001' '0001' '0000')
    for k in range(len(t)):
        out += bytes.fromhex('ffdb0043') + bytes([k]) + bytes(t[k][ref.ZZ].tolist())
    out += bytes.fromhex('ffc00011' '08') + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + bytes([3])
    out += bytes([1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, len(t) - 1])
    huffman = oref.ANNEX_K if huffman is None else huffman
    for ident, table in zip(oref.TABLE_IDS, huffman):
        n = int(np.sum(table[:16], dtype=np.int64))
        out += b'\xff\xc4' + (19 + n).to_bytes(2, 'big') + bytes([ident]) + bytes(np.asarray(table[:16 + n]).tolist())
    return out + bytes.fromhex('ffda000c' '03' '0100' '0211' '0311' '00' '3f' '00')


def decode_u8(coefs, h, w, tables, hs, vs):
    """Real-block coefficients -> the uint8 (H, W, 3) image libjpeg decodes with these tables."""
    t3 = per_component(tables)
    planes = []
    for k, c in enumerate(coefs):
        bh, bw, _ = c.shape
        nat = np.zeros((bh, bw, 64), np.int64)
        nat[..., ref.ZZ] = c.astype(np.int64)
        p = ref.idct((nat * t3[k]).reshape(bh, bw, 8, 8)).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        if k:
            p = ref._upsample(p, hs, vs, -(-h // vs), -(-w // hs))
        planes.append(p[:h, :w])
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def compress(rgb, tables, subsampling='4:4:4', optimize=False):
    """uint8 (H, W, 3) -> (the whole file, the decoded uint8 image, the flat coefficients in the device layout)."""
    hs, vs = ref.SUBSAMPLING[subsampling]
    h, w, _ = rgb.shape
    coefs = coefficients(rgb, tables, hs, vs)
    if optimize:
        huffman, status = oref.optimal_tables(oref.histograms(coefs, h, w, hs, vs))
        ecd, st = oref.entropy_code(coefs, h, w, hs, vs, huffman)
        assert not status.any() and st == 0
        data = header(h, w, tables, hs, vs, huffman) + ecd + b'\xff\xd9'
    else:
        data = header(h, w, tables, hs, vs) + ref.entropy_code(coefs, h, w, hs, vs) + b'\xff\xd9'
    return data, decode_u8(coefs, h, w, tables, hs, vs), ref.flat_coefficients(coefs)


def tables_from_float(t):
    """float tables (n_sets, n_tabs, 64) -> ((n_sets, 3, 64) uint16, (n_sets,) status): np.rint (ties to even) clamped to 1..255;
    NaN and -inf become 1, +inf 255."""
    t = np.asarray(t, np.float32)
    t = t[:, [0, 1, 1]] if t.shape[1] == 2 else t
    finite = np.isfinite(t)
    with np.errstate(invalid='ignore'):
        r = np.rint(np.where(finite, t, 1))
    raised, lowered = finite & (r < 1), finite & (r > 255)
    out = np.clip(r, 1, 255)
    out[~finite] = np.where(t[~finite] > 0, 255, 1)                  # (NaN > 0 is False)
    status = (ST_RAISED * raised.any(axis=(1, 2)) + ST_LOWERED * lowered.any(axis=(1, 2)) + ST_NONFINITE * (~finite).any(axis=(1, 2)))
    return out.astype(np.uint16), status.astype(np.int64)


def moved(t):
    """The entries tables_from_float has to clamp: JPEG.file_tables' second value."""
    t = np.asarray(t, np.float32)
    with np.errstate(invalid='ignore'):
        return ~np.isfinite(t) | (np.rint(t) < 1) | (np.rint(t) > 255)
