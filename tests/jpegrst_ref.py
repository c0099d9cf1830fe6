"""Plain Python restatement of baseline JPEG files with restart intervals (libjpeg's restart_interval, Pillow's
restart_marker_blocks): the symbols of an image with the DC predictors restarting every Ri MCUs, the histograms libjpeg's statistics
pass counts from them, the entropy-coded segment with its markers, whole files (Annex K, optimal or given Huffman tables; a quality
or given quantisation tables), and a parser that recovers the coefficients from such a file.  Built on jpeg_ref.py, jpegopt_ref.py
and jpegq_ref.py, test infrastructure like them - the product never imports it.  Ri = 0 is the file without markers."""
import numpy as np

import jpeg_ref as ref
import jpegopt_ref as oref
import jpegq_ref as qref

SITUATIONS = ('end_aligned', 'end_pad7', 'pad_makes_ff', 'data_ff_before_marker', 'markers', 'short_last_interval', 'dummy_right',
              'dummy_bottom')


def markers(h, w, hs, vs, ri):
    """How many restart markers an image carries: one behind every interval but the last."""
    my, mx = ref.geometry(h, w, hs, vs)[1]
    return -(-my * mx // ri) - 1 if ri else 0


def interval_symbols(coefs, h, w, hs, vs, ri):
    """One image in scan order, dummy blocks included, as a list of restart intervals (one interval when ri = 0), each a list of
    (table 0..3, symbol, value bits, number of value bits, kind) as jpegopt_ref.block_symbols gives them - with its clamps - and the
    DC predictors 0 at the start of every interval."""
    per = hs * vs + 2
    out, pred = [], [0, 0, 0]
    for i, (k, blk, kind) in enumerate(ref.scan_blocks(coefs, h, w, hs, vs)):
        if i % per == 0 and (i == 0 or (ri and (i // per) % ri == 0)):
            out.append([])
            pred = [0, 0, 0]
        t = 2 * min(k, 1)
        diff = min(max(int(blk[0]) - pred[k], -2047), 2047)
        pred[k] = int(blk[0])
        s = ref._category(diff)
        out[-1].append((t, s, diff if diff >= 0 else diff - 1, s, kind or 'real'))
        run = 0
        for v in blk[1:].tolist():
            if v == 0:
                run += 1
                continue
            v = min(max(v, -1023), 1023)
            while run >= 16:
                out[-1].append((t + 1, 0xf0, 0, 0, None))
                run -= 16
            s = ref._category(v)
            out[-1].append((t + 1, (run << 4) | s, v if v >= 0 else v - 1, s, None))
            run = 0
        if run:
            out[-1].append((t + 1, 0x00, 0, 0, None))
    return out


def histograms(coefs, h, w, hs, vs, ri):
    """(4, 257) uint32 - what nimg_jpeg_histogram_restart writes for one image."""
    hist = np.zeros((4, 257), np.uint32)
    for interval in interval_symbols(coefs, h, w, hs, vs, ri):
        for t, sym, _, _, _ in interval:
            hist[t, sym] += 1
    return hist


def entropy_code(coefs, h, w, hs, vs, ri, tables=None, stats=None):
    """The entropy-coded segment of one image with its four tables (4, 272), Annex K's by default: every interval padded with 1-bits
    to a byte and stuffed, FF D(k mod 8) between interval k and k + 1.  stats: a dict that counts the situations of SITUATIONS."""
    tables = oref.ANNEX_K if tables is None else tables
    codes = [oref.codes_of(tables[t], t % 2 == 0) for t in range(4)]
    assert all(ok for _, ok in codes)
    stats = stats if stats is not None else {}
    for key in SITUATIONS:
        stats.setdefault(key, 0)
    intervals = interval_symbols(coefs, h, w, hs, vs, ri)
    my, mx = ref.geometry(h, w, hs, vs)[1]
    stats['short_last_interval'] += bool(ri and len(intervals) > 1 and (my * mx) % ri)
    out = b''
    for k, interval in enumerate(intervals):
        bits = ref._Bits()
        for t, sym, value, nbits, kind in interval:
            if kind in ('right', 'bottom') and len(intervals) > 1:
                stats['dummy_' + kind] += 1
            bits.put(*codes[t][0][sym])
            bits.put(value, nbits)
        pad = (8 - bits.n) % 8
        if pad:
            bits.put(0xff, pad)
        if k + 1 < len(intervals):
            stats['end_aligned'] += pad == 0
            stats['end_pad7'] += pad == 7
            stats['pad_makes_ff'] += pad > 0 and bits.out[-1] == 0xff
            stats['data_ff_before_marker'] += pad == 0 and bits.out[-1] == 0xff
            stats['markers'] += 1
        out += bytes(bits.out).replace(b'\xff', b'\xff\x00')
        if k + 1 < len(intervals):
            out += bytes([0xff, 0xd0 | (k & 7)])
    return out


def header(h, w, qtables, hs, vs, ri, huffman=None):
    """SOI .. SOS as jpegq_ref.header, with FFDD 0004 RRRR between the last DHT segment and SOS when ri > 0."""
    base = qref.header(h, w, qtables, hs, vs, huffman)
    if not ri:
        return base
    return base[:-14] + b'\xff\xdd\x00\x04' + ri.to_bytes(2, 'big') + base[-14:]


def quality_tables(quality):
    return np.stack([ref.qtable(quality, 0), ref.qtable(quality, 1)])


def encode(coefs, h, w, qtables, hs, vs, ri, optimize=False, stats=None):
    """One image's coefficients -> (the whole file, its Huffman tables (4, 272) or None)."""
    huffman = None
    if optimize:
        huffman, status = oref.optimal_tables(histograms(coefs, h, w, hs, vs, ri))
        assert not status.any()
    ecd = entropy_code(coefs, h, w, hs, vs, ri, huffman, stats)
    return header(h, w, qtables, hs, vs, ri, huffman) + ecd + b'\xff\xd9', huffman


# ---- parser: a restart file's coefficients ------------------------------------------------------------------------------------
def split_segment(ecd):
    """A stuffed entropy-coded segment -> ([the un-stuffed bytes of each interval], [the marker numbers 0..7 between them])."""
    parts, numbers, cur, i = [], [], bytearray(), 0
    while i < len(ecd):
        b = ecd[i]
        if b == 0xff:
            nxt = ecd[i + 1]
            if nxt == 0:
                cur.append(0xff)
            elif 0xd0 <= nxt <= 0xd7:
                parts.append(bytes(cur))
                numbers.append(nxt - 0xd0)
                cur = bytearray()
            else:
                raise ValueError('marker FF{:02X} in the entropy-coded segment'.format(nxt))
            i += 2
        else:
            cur.append(b)
            i += 1
    parts.append(bytes(cur))
    return parts, numbers


def parse(data):
    """A baseline file with or without restart markers -> dict(h, w, hs, vs, ri, qtables (3, 64) per component in natural order,
    huffman {id byte: (counts, symbols)}, ecd_offset, coefs [Y, Cb, Cr] over the REAL blocks, (rows, cols, 64) int16 zig-zag).  The
    markers must be exactly those the interval asks for, in sequence, and every interval must end in at most 7 one-bits."""
    assert data[:2] == b'\xff\xd8' and data[-2:] == b'\xff\xd9'
    i, q, huff, info = 2, {}, {}, {'ri': 0}
    while True:
        marker, length = data[i:i + 2], int.from_bytes(data[i + 2:i + 4], 'big')
        body = data[i + 4:i + 2 + length]
        if marker == b'\xff\xdb':
            while body:
                q[body[0] & 15] = np.zeros(64, np.int64)
                q[body[0] & 15][ref.ZZ] = list(body[1:65])
                body = body[65:]
        elif marker == b'\xff\xc0':
            info['h'], info['w'] = int.from_bytes(body[1:3], 'big'), int.from_bytes(body[3:5], 'big')
            info['hs'], info['vs'] = body[7] >> 4, body[7] & 15
            selectors = [body[8 + 3 * c] for c in range(3)]
        elif marker == b'\xff\xc4':
            while body:
                n = sum(body[1:17])
                huff[body[0]] = (bytes(body[1:17]), bytes(body[17:17 + n]))
                body = body[17 + n:]
        elif marker == b'\xff\xdd':
            info['ri'] = int.from_bytes(body, 'big')
        elif marker == b'\xff\xda':
            i += 2 + length
            break
        i += 2 + length
    info['ecd_offset'], info['huffman'] = i, huff
    info['qtables'] = np.stack([q[s] for s in selectors])
    h, w, hs, vs, ri = info['h'], info['w'], info['hs'], info['vs'], info['ri']
    comps, (my, mx) = ref.geometry(h, w, hs, vs)
    parts, numbers = split_segment(data[i:-2])
    assert numbers == [k & 7 for k in range(markers(h, w, hs, vs, ri))], (numbers, ri)
    tables = {}
    for ident, (counts, symbols) in huff.items():
        table, code, k = {}, 0, 0
        for ln in range(1, 17):
            for _ in range(counts[ln - 1]):
                table[(code, ln)] = symbols[k]
                code, k = code + 1, k + 1
            code <<= 1
        tables[ident] = table
    full = [np.zeros((my * cv, mx * ch, 64), np.int16) for ch, cv in ((hs, vs), (1, 1), (1, 1))]
    mcu = 0
    for part in parts:
        bits, pos, pred = ''.join('{:08b}'.format(b) for b in part), 0, [0, 0, 0]

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

        for _ in range(min(ri, my * mx - mcu) if ri else my * mx):
            r, c = divmod(mcu, mx)
            for k, (ch, cv) in enumerate(((hs, vs), (1, 1), (1, 1))):
                t = min(k, 1)
                for dy in range(cv):
                    for dx in range(ch):
                        blk = full[k][r * cv + dy, c * ch + dx]
                        pred[k] += value(symbol(tables[t]))
                        blk[0] = pred[k]
                        j = 1
                        while j < 64:
                            rs = symbol(tables[0x10 | t])
                            if rs == 0:
                                break
                            j += rs >> 4
                            if rs & 15:
                                blk[j] = value(rs & 15)
                            j += 1
            mcu += 1
        assert len(bits) - pos < 8 and all(b == '1' for b in bits[pos:])
    assert mcu == my * mx
    info['coefs'] = [full[k][:comps[k][2], :comps[k][3]].copy() for k in range(3)]
    return info
