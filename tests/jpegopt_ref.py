"""Plain Python restatement of JPEG files with optimised Huffman tables (libjpeg's optimize_coding, Pillow's
optimize=True): the symbol histograms of a coefficient set, libjpeg's jpeg_gen_optimal_table, the codes of a DHT body, entropy
coding with given tables and the header with per-image DHT segments.  Built on jpeg_ref.py, test infrastructure like it - the product
never imports it.  A table is the 272 bytes nimg_jpeg_decode takes: 16 counts, then 256 symbol bytes in code order, unused ones 0;
the four tables of an image stand in DHT-id order 00 (Y DC), 10 (Y AC), 01 (chroma DC), 11 (chroma AC)."""
import numpy as np

import jpeg_ref as ref

TABLE_IDS = (0x00, 0x10, 0x01, 0x11)
TABLE_BYTES = 272
ST_OVERFLOW, ST_TOTAL = 1, 2                # nimg_jpeg_optimal_tables: a code size above 32 | a histogram total of 2^32 or more
ST_TABLE, ST_SYMBOL = 1, 2                  # nimg_jpeg_encode_tables: counts that are no prefix code | a used symbol without a code


def block_symbols(coefs, h, w, hs, vs):
    """One image in scan order, dummy blocks included: [(table 0..3, symbol, value bits, number of value bits, kind)] with the clamps
    of nimg_jpeg_encode (DC difference +-2047, AC +-1023); kind as jpeg_ref.scan_blocks, on the DC symbol of a block."""
    out, pred = [], [0, 0, 0]
    for k, blk, kind in ref.scan_blocks(coefs, h, w, hs, vs):
        t = 2 * min(k, 1)
        diff = min(max(int(blk[0]) - pred[k], -2047), 2047)
        pred[k] = int(blk[0])
        s = ref._category(diff)
        out.append((t, s, diff if diff >= 0 else diff - 1, s, kind or 'real'))
        run = 0
        for v in blk[1:].tolist():
            if v == 0:
                run += 1
                continue
            v = min(max(v, -1023), 1023)
            while run >= 16:
                out.append((t + 1, 0xf0, 0, 0, None))
                run -= 16
            s = ref._category(v)
            out.append((t + 1, (run << 4) | s, v if v >= 0 else v - 1, s, None))
            run = 0
        if run:
            out.append((t + 1, 0x00, 0, 0, None))
    return out


def histograms(coefs, h, w, hs, vs):
    """(4, 257) uint32 - what nimg_jpeg_histogram writes for one image; entry 256 is 0."""
    hist = np.zeros((4, 257), np.uint32)
    for t, sym, _, _, _ in block_symbols(coefs, h, w, hs, vs):
        hist[t, sym] += 1
    return hist


def limit_bits(bits):
    """Annex K.3 on bits[0..32] in place (sizes above 16 folded back), then the pseudo-symbol removed."""
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while j > 1 and bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while i > 1 and bits[i] == 0:
        i -= 1
    if bits[i] > 0:
        bits[i] -= 1


def code_sizes(hist):
    """The unlimited code size of each of the 257 entries (the pseudo-symbol 256 included), by libjpeg's merging."""
    freq = [int(v) for v in hist[:256]] + [1]
    size, tree = [0] * 257, list(range(257))
    while True:
        c1 = c2 = -1
        for i in range(257):
            if freq[i] and (c1 < 0 or freq[i] <= freq[c1]):
                c1 = i
        for i in range(257):
            if freq[i] and i != c1 and (c2 < 0 or freq[i] <= freq[c2]):
                c2 = i
        if c2 < 0:
            return size
        freq[c1] += freq[c2]
        freq[c2] = 0
        for i in range(257):
            if tree[i] == c1 or tree[i] == c2:
                size[i] += 1
                tree[i] = c1


def optimal_table(hist):
    """A 257-entry histogram -> (table (272,) uint8, status) as nimg_jpeg_optimal_tables gives them."""
    table = np.zeros(TABLE_BYTES, np.uint8)
    total = sum(int(v) for v in hist[:256])
    if total + 1 >= 1 << 32:
        return table, ST_TOTAL
    if total == 0:
        return table, 0
    size = code_sizes(hist)
    if max(size) > 32:
        return table, ST_OVERFLOW
    bits = [0] * 33
    for s in size:
        if s:
            bits[s] += 1
    limit_bits(bits)
    table[:16] = bits[1:17]
    symbols = [v for s in range(1, 33) for v in range(256) if size[v] == s]
    table[16:16 + len(symbols)] = symbols
    return table, 0


def optimal_tables(hists):
    """(m, 257) -> ((m, 272) uint8, (m,) status)."""
    done = [optimal_table(h) for h in np.asarray(hists).reshape(-1, 257)]
    return np.stack([d[0] for d in done]), np.array([d[1] for d in done], np.int64)


def table_of(counts, symbols):
    """(16 counts, symbols in code order) as bytes or sequences -> (272,) uint8."""
    table = np.zeros(TABLE_BYTES, np.uint8)
    table[:16] = list(counts)
    table[16:16 + len(symbols)] = list(symbols)
    return table


ANNEX_K = np.stack([table_of(ref.HUFF[t][0], bytes.fromhex(ref.HUFF[t][1])) for t in TABLE_IDS])


def codes_of(table, dc):
    """One table -> ({symbol: (code, length)}, valid).  valid is the decoder's check: at most 256 symbols, and the counts a prefix
    code of lengths 1..16.  A DC table keeps the symbols below 16 only; of a symbol listed twice the last code counts."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        cnt = int(table[length - 1])
        if k + cnt > 256 or code + cnt > (1 << length):
            return {}, False
        for j in range(cnt):
            sym = int(table[16 + k + j])
            if not dc or sym < 16:
                codes[sym] = (code + j, length)
        k += cnt
        code = (code + cnt) << 1
    return codes, True


def entropy_code(coefs, h, w, hs, vs, tables):
    """The entropy-coded segment of one image with its four tables (4, 272) -> (bytes, status) as nimg_jpeg_encode_tables."""
    codes = [codes_of(tables[t], t % 2 == 0) for t in range(4)]
    if not all(ok for _, ok in codes):
        return b'', ST_TABLE
    bits, status = ref._Bits(), 0
    for t, sym, value, nbits, _ in block_symbols(coefs, h, w, hs, vs):
        if sym not in codes[t][0]:
            status |= ST_SYMBOL                 # no code: the symbol and its value bits are left out
            continue
        bits.put(*codes[t][0][sym])
        bits.put(value, nbits)
    if bits.n:
        bits.put(0xff, 8 - bits.n)
    return bytes(bits.out).replace(b'\xff', b'\xff\x00'), status


def header(h, w, quality, hs, vs, tables):
    """SOI .. SOS with the four tables (4, 272) in DHT segments of their own, in the order 00 10 01 11."""
    base = ref.header(h, w, quality, hs, vs)
    at = base.index(b'\xff\xc4')
    assert at == 177
    out = base[:at]
    for ident, table in zip(TABLE_IDS, tables):
        n = int(np.sum(table[:16], dtype=np.int64))
        out += b'\xff\xc4' + (19 + n).to_bytes(2, 'big') + bytes([ident]) + bytes(table[:16 + n].tolist())
    return out + base[-14:]


def encode(coefs, h, w, quality, hs, vs):
    """One image's coefficients -> (the whole optimised file, its tables (4, 272), its histograms (4, 257), its segment)."""
    hist = histograms(coefs, h, w, hs, vs)
    tables, status = optimal_tables(hist)
    assert not status.any()
    ecd, st = entropy_code(coefs, h, w, hs, vs, tables)
    assert st == 0
    return header(h, w, quality, hs, vs, tables) + ecd + b'\xff\xd9', tables, hist, ecd


def tables_of_file(data):
    """The four tables (4, 272) of a file in the order Y DC, Y AC, chroma DC, chroma AC as its scan assigns them (Cb's)."""
    import jpegd_ref
    return jpegd_ref.huffman_bytes(jpegd_ref.header(data))[:4]
