"""Plain numpy / Python restatement of grey-scale JPEG files (what libjpeg writes and reads for a mode 'L'
image): one component, no colour conversion, the blocks in raster order over ceil(h / 8) x ceil(w / 8) with the right and bottom edges
replicated, one block per MCU, so that a restart interval counts blocks.  Writer (Annex K, optimal or given Huffman tables, a restart
interval), header, a parser by the markers alone, the decoder to pixels, a progressive writer for any legal one-component script and
the models of both GPU decoders with the one-component geometry.  Built on jpeg_ref.py, jpegopt_ref.py, jpegd_ref.py, jpegprog_ref.py
and jpegdprog_ref.py, test infrastructure like them - the product never imports it.  A coefficient set is (block rows, block cols, 64)
int16 in zig-zag order; an image's two tables stand in the order DC, AC (the DHT ids 00 10)."""
import numpy as np

import jpeg_ref as ref
import jpegd_ref as dref
import jpegdprog_ref as dpref
import jpegopt_ref as oref
import jpegprog_ref as pref

ANNEX_K = oref.ANNEX_K[:2]                  # (2, 272): the luma tables
HEADER_BYTES, DHT_OFFSET = 328, 102
C0 = (0,)
# libjpeg's jpeg_simple_progression for one component (Pillow's progressive=True on an 'L' image)
SCRIPT_STD = ((C0, 0, 0, 0, 1), (C0, 1, 5, 0, 2), (C0, 6, 63, 0, 2), (C0, 1, 63, 2, 1), (C0, 0, 0, 1, 0), (C0, 1, 63, 1, 0))
# a second legal script: the DC in one scan, the AC split in three bands, two refinements
SCRIPT_BANDS = ((C0, 0, 0, 0, 0), (C0, 1, 5, 0, 1), (C0, 6, 20, 0, 1), (C0, 21, 63, 0, 0), (C0, 1, 5, 1, 0), (C0, 6, 20, 1, 0))


def geometry(h, w):
    """(block rows, block cols)"""
    return -(-h // 8), -(-w // 8)


def markers(h, w, ri):
    bh, bw = geometry(h, w)
    return -(-bh * bw // ri) - 1 if ri else 0


def coefficients(img, qtable):
    """uint8 (H, W) and the table (64,) in natural order -> (block rows, block cols, 64) int16, zig-zag."""
    h, w = img.shape
    bh, bw = geometry(h, w)
    p = np.pad(img.astype(np.int64), ((0, 8 * bh - h), (0, 8 * bw - w)), mode='edge')
    x = ref.fdct(p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)).reshape(bh, bw, 64)
    qv = np.asarray(qtable, np.int64) << 3
    c = np.sign(x) * ((np.abs(x) + (qv >> 1)) // qv)
    return c[..., ref.ZZ].astype(np.int16)


def decode_u8(coef, qtable, h, w):
    """Coefficients -> the uint8 (H, W) image libjpeg decodes: islow inverse DCT and the range limit, nothing else."""
    bh, bw, _ = coef.shape
    nat = np.zeros((bh, bw, 64), np.int64)
    nat[..., ref.ZZ] = coef.astype(np.int64)
    x = ref.idct((nat * np.asarray(qtable, np.int64)).reshape(bh, bw, 8, 8))
    return x.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)[:h, :w].astype(np.uint8)


def interval_symbols(coef, ri):
    """One image in raster order as a list of restart intervals (one when ri = 0), each a list of (table 0 DC | 1 AC, symbol, value bits,
    their number), with the coder's clamps and the DC predictor 0 at the start of every interval."""
    out, pred = [], 0
    for i, blk in enumerate(coef.reshape(-1, 64)):
        if i == 0 or (ri and i % ri == 0):
            out.append([])
            pred = 0
        diff = min(max(int(blk[0]) - pred, -2047), 2047)
        pred = int(blk[0])
        s = ref._category(diff)
        out[-1].append((0, s, diff if diff >= 0 else diff - 1, s))
        run = 0
        for v in blk[1:].tolist():
            if v == 0:
                run += 1
                continue
            v = min(max(v, -1023), 1023)
            while run >= 16:
                out[-1].append((1, 0xf0, 0, 0))
                run -= 16
            s = ref._category(v)
            out[-1].append((1, (run << 4) | s, v if v >= 0 else v - 1, s))
            run = 0
        if run:
            out[-1].append((1, 0x00, 0, 0))
    return out


def histograms(coef, ri=0):
    """(2, 257) uint32 - what nimg_jpeg_grey_histogram writes for one image."""
    hist = np.zeros((2, 257), np.uint32)
    for interval in interval_symbols(coef, ri):
        for t, sym, _, _ in interval:
            hist[t, sym] += 1
    return hist


def entropy_code(coef, ri=0, tables=None):
    """The entropy-coded segment of one image with its two tables (2, 272), Annex K's by default -> (bytes, status) as
    nimg_jpeg_grey_encode_tables: every interval padded with 1-bits and stuffed, FF D(k mod 8) between interval k and k + 1."""
    tables = ANNEX_K if tables is None else tables
    codes = [oref.codes_of(tables[t], t == 0) for t in range(2)]
    intervals = interval_symbols(coef, ri)
    if not all(ok for _, ok in codes):
        return b''.join(bytes([0xff, 0xd0 | (k & 7)]) for k in range(len(intervals) - 1)), oref.ST_TABLE
    out, status = b'', 0
    for k, interval in enumerate(intervals):
        bits = ref._Bits()
        for t, sym, value, nbits in interval:
            if sym not in codes[t][0]:
                status |= oref.ST_SYMBOL
                continue
            bits.put(*codes[t][0][sym])
            bits.put(value, nbits)
        if bits.n:
            bits.put(0xff, 8 - bits.n)
        out += bytes(bits.out).replace(b'\xff', b'\xff\x00')
        if k + 1 < len(intervals):
            out += bytes([0xff, 0xd0 | (k & 7)])
    return out, status


def header(h, w, qtable, ri=0, huffman=None, sampling=0x11, progressive=False):
    """SOI .. SOS of a baseline file (328 bytes with the Annex K tables, a DRI segment 6 more); progressive: SOI .. SOF2 alone."""
    out = bytes.fromhex('ffd8' 'ffe00010' '4a46494600' '0101' '00' '0001' '0001' '0000')
    out += bytes.fromhex('ffdb0043' '00') + bytes(np.asarray(qtable, np.int64)[ref.ZZ].astype(np.uint8).tolist())
    out += (b'\xff\xc2' if progressive else b'\xff\xc0') + bytes.fromhex('000b' '08') + h.to_bytes(2, 'big') + w.to_bytes(2, 'big')
    out += bytes([1, 1, sampling, 0])
    if progressive:
        return out
    for ident, table in zip((0x00, 0x10), ANNEX_K if huffman is None else huffman):
        out += pref.dht(ident, table)
    if ri:
        out += b'\xff\xdd\x00\x04' + int(ri).to_bytes(2, 'big')
    return out + bytes.fromhex('ffda0008' '01' '0100' '00' '3f' '00')


def encode(coef, h, w, qtable, ri=0, optimize=False, sampling=0x11):
    """One image's coefficients -> (the whole file, its Huffman tables (2, 272) or None)."""
    huffman = None
    if optimize:
        huffman, status = oref.optimal_tables(histograms(coef, ri))
        assert not status.any()
    ecd, st = entropy_code(coef, ri, huffman)
    assert st == 0
    return header(h, w, qtable, ri, huffman, sampling) + ecd + b'\xff\xd9', huffman


# ---- progressive files of one component ------------------------------------------------------------------------------------------
def _sos(ss, se, ah, al):
    return bytes([0xff, 0xda, 0, 8, 1, 1, 0, ss, se, (ah << 4) | al])


def encode_progressive(coef, h, w, qtable, script=SCRIPT_STD, ri=0, sampling=0x11):
    """One image's coefficients -> the whole progressive file of `script`: every scan but a DC refine one with the optimal table of its
    own symbols in a DHT segment in front of it (id 00 for the DC, 10 for every AC table), as libjpeg writes a one-component file.
    jpegprog_ref's walks, which read the script from the module's SCANS."""
    rows = [(C0, ss, se, ah, al, None, None if ss == 0 and ah else t) for t, (_, ss, se, ah, al) in enumerate(script)]
    saved = pref.SCANS
    pref.SCANS = tuple(rows)
    try:
        items = [pref.scan_items([coef], h, w, 1, 1, i, ri) for i in range(len(rows))]
    finally:
        pref.SCANS = saved
    hist = np.zeros((len(rows), 257), np.uint32)
    for scan in items:
        for it in scan:
            if it[0] == 'sym':
                hist[it[1], it[2]] += 1
    tables, status = oref.optimal_tables(hist)
    assert not status.any()
    out = header(h, w, qtable, sampling=sampling, progressive=True)
    for k, (row, scan) in enumerate(zip(rows, items)):
        # code_segment takes a DC table for table indices below 2: a DC symbol is below 12, so an AC scan whose index is 0 or 1 (never
        # here: scan 0 is the DC first scan, and 1 is DC only in no legal script) would lose nothing either
        seg, st = _code_segment(scan, tables, row[1] == 0)
        assert st == 0
        if row[6] is not None:
            out += pref.dht(0x10 if row[1] else 0x00, tables[row[6]])
        if k == 0 and ri:
            out += b'\xff\xdd\x00\x04' + int(ri).to_bytes(2, 'big')
        out += _sos(*row[1:5]) + seg
    return out + b'\xff\xd9'


def _code_segment(items, tables, dc):
    """jpegprog_ref.code_segment with the table's kind given instead of read off its index."""
    bits, out, status, codes = ref._Bits(), b'', 0, {}

    def pad():
        if bits.n:
            bits.put(0xff, 8 - bits.n)
        return bytes(bits.out).replace(b'\xff', b'\xff\x00')

    for it in items:
        if it[0] == 'sym':
            if it[1] not in codes:
                codes[it[1]] = oref.codes_of(tables[it[1]], dc)[0]
            if it[2] not in codes[it[1]]:
                status |= oref.ST_SYMBOL
                continue
            bits.put(*codes[it[1]][it[2]])
            bits.put(it[3], it[4])
        elif it[0] == 'bits':
            bits.put(it[1], it[2])
        else:
            out += pad() + bytes([0xff, 0xd0 + it[1]])
            bits = ref._Bits()
    return out + pad(), status


# ---- a file by its markers ---------------------------------------------------------------------------------------------------------
def split(data):
    """A grey-scale file, baseline or progressive -> dict(h, w, sampling, progressive, ri, qtable (64,) natural order, script, tables =
    per scan [(counts, symbols) DC, AC] (baseline) or [(counts, symbols)] (a progressive scan; (16 zeros, b'') for a DC refine one),
    segments = per scan the stuffed bytes with their restart markers, ecd_offset = where the first begins)."""
    assert data[:2] == b'\xff\xd8' and data[-2:] == b'\xff\xd9'
    i, q, dht, out = 2, {}, {}, dict(ri=0, script=[], tables=[], segments=[])
    while data[i:i + 2] != b'\xff\xd9':
        marker, length = data[i + 1], int.from_bytes(data[i + 2:i + 4], 'big')
        body = data[i + 4:i + 2 + length]
        i += 2 + length
        if marker == 0xdb:
            while body:
                q[body[0] & 15] = np.zeros(64, np.int64)
                q[body[0] & 15][ref.ZZ] = list(body[1:65])
                body = body[65:]
        elif marker in (0xc0, 0xc2):
            assert body[5] == 1, 'not a one-component frame'
            out['h'], out['w'] = int.from_bytes(body[1:3], 'big'), int.from_bytes(body[3:5], 'big')
            out['sampling'], out['progressive'], tq = body[7], marker == 0xc2, body[8]
        elif marker == 0xc4:
            while body:
                n = sum(body[1:17])
                dht[body[0]] = (bytes(body[1:17]), bytes(body[17:17 + n]))
                body = body[17 + n:]
        elif marker == 0xdd:
            out['ri'] = int.from_bytes(body, 'big')
        elif marker == 0xda:
            assert body[0] == 1
            sel, ss, se, ah, al = body[2], body[3], body[4], body[5] >> 4, body[5] & 15
            out['script'].append((C0, ss, se, ah, al))
            if not out['progressive']:
                out['tables'].append([dht[sel >> 4], dht[0x10 | (sel & 15)]])
            else:
                out['tables'].append([(bytes(16), b'') if ss == 0 and ah else dht[(sel >> 4) if ss == 0 else 0x10 | (sel & 15)]])
            out.setdefault('ecd_offset', i)
            j = i
            while not (data[j] == 0xff and data[j + 1] != 0 and not 0xd0 <= data[j + 1] <= 0xd7):
                j += 1
            out['segments'].append(data[i:j])
            i = j
    out['qtable'] = q[tq]
    return out


def table_bytes(pairs, slots=None):
    """[(counts, symbols)] -> (len(pairs) or `slots`, 272) uint8."""
    out = np.zeros((slots or len(pairs), 272), np.uint8)
    for t, (counts, symbols) in enumerate(pairs):
        out[t, :16] = list(counts)
        out[t, 16:16 + len(symbols)] = list(symbols)
    return out


# ---- the models of the decoders with the one-component geometry ------------------------------------------------------------------------
class Geometry(object):
    """jpegdprog_ref.Geometry for a frame of one component: every scan is a one-component scan over its blocks in raster order."""

    def __init__(self, h, w, ri):
        bh, bw = geometry(h, w)
        self.hs = self.vs = self.per = 1
        self.my, self.mx, self.ri = bh, bw, ri
        self.shapes, self.base, self.SB = [(bh, bw)], [0, bh * bw], bh * bw

    def scan(self, cs):
        span = self.ri if self.ri else self.SB
        return self.SB, 1, span, -(-self.SB // span)

    def place(self, cs, b):
        return 0, b


def decode_progressive(data, subseq_bits=0):
    """A progressive grey-scale file -> (flat int16 coefficients, status, [rounds per scan]); the scans level after level."""
    p = split(data)
    geo = Geometry(p['h'], p['w'], p['ri'])
    coef = np.zeros(geo.SB * 64, np.int64)
    lv = dpref.levels(p['script'])
    status, rounds = 0, [0] * len(lv)
    for level in range(1, max(lv) + 1):
        for s, scan in enumerate(p['script']):
            if lv[s] != level:
                continue
            model = dpref.Scan(geo, scan, p['tables'][s], p['segments'][s], coef)
            if scan[3] == 0:
                rounds[s] = model.run_first(subseq_bits)
            elif scan[1] == 0:
                model.run_dc_refine()
            else:
                model.run_ac_refine()
            status |= model.status
    return coef.astype(np.int16), status, rounds


class Model(dref.Model):
    """jpegd_ref.Model - the parallel baseline decoder of a file without restart markers - over one component: every block of the scan
    is block 0 of its MCU and a real one.  run(subseq_bits) -> (flat coefficients, status, rounds, subsequences)."""

    def __init__(self, h, w, tables, ecd):
        dref.Model.__init__(self, 8, 8, 1, 1, list(tables) * 3, ecd)       # (the bit string and the look-ups; the geometry follows)
        bh, bw = geometry(h, w)
        self.per, self.mx, self.SB = 1, bw, bh * bw
        self.shapes, self.base = [(bh, bw)], [0, bh * bw, bh * bw, bh * bw]

    def place(self, b):
        return 0, b

    def decode(self, state, limit, write=None):
        # the base class derives the luma blocks of an MCU as per - 2: one here
        self.per = 3
        try:
            state, begun = dref.Model.decode(self, None if state is None else (state[0], 0, state[2]), limit, write)
        finally:
            self.per = 1
        return (None if state is None else (state[0], 0, state[2])), begun


def decode_baseline(data):
    """A baseline grey-scale file, with or without restart markers -> the (block rows, block cols, 64) int16 coefficients, by a plain
    sequential walk: the markers must be exactly those the interval asks for, every interval must end in at most 7 one-bits."""
    import jpegrst_ref as rref
    p = split(data)
    assert not p['progressive'] and p['script'] == [(C0, 0, 63, 0, 0)]
    bh, bw = geometry(p['h'], p['w'])
    parts, numbers = rref.split_segment(p['segments'][0])
    assert numbers == [k & 7 for k in range(markers(p['h'], p['w'], p['ri']))], (numbers, p['ri'])
    tables = []
    for counts, symbols in p['tables'][0]:
        table, code, k = {}, 0, 0
        for ln in range(1, 17):
            for _ in range(counts[ln - 1]):
                table[(code, ln)] = symbols[k]
                code, k = code + 1, k + 1
            code <<= 1
        tables.append(table)
    coef, b = np.zeros((bh * bw, 64), np.int16), 0
    for part in parts:
        bits, pos, pred = ''.join('{:08b}'.format(v) for v in part), 0, 0

        def symbol(table):
            nonlocal pos
            code = 0
            for ln in range(1, 17):
                code = (code << 1) | (bits[pos + ln - 1] == '1')
                if (code, ln) in table:
                    pos += ln
                    return table[(code, ln)]
            raise ValueError('bad Huffman code at bit {}'.format(pos))

        def value(s):
            nonlocal pos
            if s == 0:
                return 0
            v = int(bits[pos:pos + s], 2)
            pos += s
            return v if v >> (s - 1) else v - (1 << s) + 1

        for _ in range(min(p['ri'], bh * bw - b) if p['ri'] else bh * bw):
            pred += value(symbol(tables[0]))
            coef[b, 0] = pred
            j = 1
            while j < 64:
                rs = symbol(tables[1])
                if rs == 0:
                    break
                j += rs >> 4
                if rs & 15:
                    coef[b, j] = value(rs & 15)
                j += 1
            b += 1
        assert len(bits) - pos < 8 and all(v == '1' for v in bits[pos:])
    assert b == bh * bw
    return coef.reshape(bh, bw, 64)
