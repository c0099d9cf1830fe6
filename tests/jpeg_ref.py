"""Plain numpy / Python restatement of the baseline JPEG codec of DESIGN.md section 4c (the format libjpeg writes with default
settings): encoder (whole files), decoder from coefficients, and a small Huffman parser that recovers the coefficients from a
file.  Test infrastructure like l3ic_ref.py - the product never imports it.  Everything is integer arithmetic; the only float
step is the final float32(u8) / float32(255)."""
import numpy as np

# Annex K Huffman tables: (number of codes of length 1..16, symbols in code order), keyed by the DHT id byte
HUFF = {
    0x00: ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], '000102030405060708090a0b'),
    0x10: ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738'
           '393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5'
           'a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa'),
    0x01: ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], '000102030405060708090a0b'),
    0x11: ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
           '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637'
           '38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3'
           'a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa'),
}
SUBSAMPLING = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}
HEADER_BYTES = 623

LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
        80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
        95, 98, 112, 100, 103, 99]
CHROMA = [17, 18, 24, 47] + [99] * 4 + [18, 21, 26, 66] + [99] * 4 + [24, 26, 56] + [99] * 5 + [47, 66] + [99] * 38


def _zigzag():
    order = sorted(range(64), key=lambda k: (k // 8 + k % 8, (k // 8) if (k // 8 + k % 8) % 2 else -(k // 8)))
    return np.array(order)


ZZ = _zigzag()                      # ZZ[scan position] = natural index 8 * row + col


def qtable(quality, channel):
    """libjpeg's table (jpeg_quality_scaling + jpeg_add_quant_table, integer arithmetic), natural order, int64 (64,)."""
    quality = min(100, max(1, int(quality)))
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    t = (np.array(LUMA if channel == 0 else CHROMA, np.int64) * scale + 50) // 100
    return np.clip(t, 1, 255)


def huff_codes(table_id):
    """symbol -> (code, length) of one Annex K table."""
    bits, vals = HUFF[table_id]
    vals = bytes.fromhex(vals)
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def to_bytes(x):
    """The reference's conversion of a float batch to bytes (float32 multiply, truncation); clamps where numpy would wrap."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return x
    x = x.astype(np.float32)
    if x.max() > 1:
        x = x / np.float32(255)
    return np.clip(np.trunc(np.float32(255) * x), 0, 255).astype(np.uint8)


def geometry(h, w, hs, vs):
    """Per component (Y, Cb, Cr): (h factor, v factor, real block rows, real block cols); and the MCU grid (rows, cols)."""
    mcus = (-(-h // (8 * vs)), -(-w // (8 * hs)))
    comps = []
    for ch, cv in ((hs, vs), (1, 1), (1, 1)):
        ce_h, ce_w = -(-h * cv // vs), -(-w * ch // hs)
        comps.append((ch, cv, -(-ce_h // 8), -(-ce_w // 8)))
    return comps, mcus


def _D(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, n, first):
    d = [d[..., k] for k in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _D(t10 + t11, 2), _D(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2], o[6] = _D(z1 + t13 * 6270, n), _D(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _D(t4 + z1 + z3, n), _D(t5 + z2 + z4, n), _D(t6 + z2 + z3, n), _D(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct(blocks):
    """(..., 8, 8) samples 0..255 -> 8 x DCT, int64 (libjpeg jfdctint)."""
    d = blocks.astype(np.int64) - 128
    d = _fdct_pass(d, 11, True)                                     # rows
    return np.swapaxes(_fdct_pass(np.swapaxes(d, -1, -2), 15, False), -1, -2)


def _idct_pass(i, n):
    i = [i[..., k] for k in range(8)]
    z1 = (i[2] + i[6]) * 4433
    t2, t3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    o = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return np.stack([_D(v, n) for v in o], axis=-1)


def idct(coef):
    """(..., 8, 8) dequantised coefficients -> samples 0..255 (libjpeg jidctint)."""
    c = np.swapaxes(_idct_pass(np.swapaxes(coef.astype(np.int64), -1, -2), 11), -1, -2)      # columns
    return np.clip(_idct_pass(c, 18) + 128, 0, 255)


def component_planes(rgb, hs, vs):
    """uint8 (H, W, 3) -> the three sample planes as the forward DCT sees them, padded to whole MCUs."""
    h, w, _ = rgb.shape
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    wp, hp, hv = -(-w // (8 * hs)) * 8 * hs, -(-h // (8 * vs)) * 8 * vs, -(-h // vs) * vs
    out = []
    for k, p in enumerate((y, cb, cr)):
        p = np.pad(p, ((0, hv - h), (0, wp - w)), mode='edge')
        if k and hs == 2:
            bias = np.arange(wp // 2) & 1
            if vs == 2:
                p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 1 + bias) >> 2
            else:
                p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        rows = hp // (vs if k else 1)
        out.append(np.pad(p, ((0, rows - p.shape[0]), (0, 0)), mode='edge'))
    return out


def coefficients(rgb, quality, hs, vs):
    """uint8 (H, W, 3) -> [Y, Cb, Cr] quantised coefficients (block rows, block cols, 64 in zig-zag order) of the REAL blocks."""
    comps, _ = geometry(rgb.shape[0], rgb.shape[1], hs, vs)
    out = []
    for k, p in enumerate(component_planes(rgb, hs, vs)):
        bh, bw = p.shape[0] // 8, p.shape[1] // 8
        x = fdct(p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)).reshape(bh, bw, 64)
        qv = qtable(quality, min(k, 1)) << 3
        c = np.sign(x) * ((np.abs(x) + (qv >> 1)) // qv)
        out.append(c[:comps[k][2], :comps[k][3]][..., ZZ].astype(np.int16))
    return out


def flat_coefficients(coefs):
    """[image][component][block row][block col][64] as one int16 vector (the layout of the device tensor, one image)."""
    return np.concatenate([c.reshape(-1) for c in coefs])


def _category(v):
    return int(abs(int(v))).bit_length()


class _Bits(object):
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xff)
        self.acc &= (1 << self.n) - 1


def scan_blocks(coefs, h, w, hs, vs):
    """The blocks of one image in scan order, dummies included: list of (component, 64 coefficients, kind) with kind
    None | 'right' | 'bottom'."""
    comps, (my, mx) = geometry(h, w, hs, vs)
    blocks = []
    for r in range(my):
        for c in range(mx):
            for k, (ch, cv, bh, bw) in enumerate(comps):
                last = None
                for dy in range(cv):
                    for dx in range(ch):
                        br, bc = r * cv + dy, c * ch + dx
                        if br < bh and bc < bw:
                            last = coefs[k][br, bc]
                            blocks.append((k, last, None))
                        else:
                            dummy = np.zeros(64, np.int16)
                            dummy[0] = last[0]
                            blocks.append((k, dummy, 'bottom' if br >= bh else 'right'))
    return blocks


def entropy_code(coefs, h, w, hs, vs, stats=None):
    """The entropy-coded segment (stuffed, padded with 1-bits) of one image."""
    dc = [huff_codes(0x00), huff_codes(0x01)]
    ac = [huff_codes(0x10), huff_codes(0x11)]
    bits, pred = _Bits(), [0, 0, 0]
    stats = stats if stats is not None else {}
    for key in ('stuffed', 'zrl', 'ac10', 'dc11', 'dummy_right', 'dummy_bottom', 'pad_some', 'pad_none'):
        stats.setdefault(key, 0)
    for k, blk, kind in scan_blocks(coefs, h, w, hs, vs):
        t = min(k, 1)
        if kind:
            stats['dummy_' + kind] += 1
        diff = int(blk[0]) - pred[k]
        pred[k] = int(blk[0])
        s = _category(diff)
        stats['dc11'] += s == 11
        bits.put(*dc[t][s])
        bits.put(diff if diff >= 0 else diff - 1, s)
        run = 0
        for v in blk[1:].tolist():
            if v == 0:
                run += 1
                continue
            while run >= 16:
                bits.put(*ac[t][0xf0])
                stats['zrl'] += 1
                run -= 16
            s = _category(v)
            stats['ac10'] += s == 10
            bits.put(*ac[t][(run << 4) | s])
            bits.put(v if v >= 0 else v - 1, s)
            run = 0
        if run:
            bits.put(*ac[t][0x00])
    stats['pad_some' if bits.n else 'pad_none'] += 1
    if bits.n:
        bits.put(0xff, 8 - bits.n)
    stats['stuffed'] += bits.out.count(0xff)
    return bytes(bits.out).replace(b'\xff', b'\xff\x00')


def header(h, w, quality, hs, vs):
    """The 623 bytes in front of the entropy-coded segment."""
    out = bytes.fromhex('ffd8' 'ffe00010' '4a46494600' '0101' '00' '0001' '0001' '0000')
    for t in (0, 1):
        out += bytes.fromhex('ffdb0043') + bytes([t]) + bytes(qtable(quality, t)[ZZ].astype(np.uint8).tolist())
    out += bytes.fromhex('ffc00011' '08') + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + bytes([3])
    out += bytes([1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1])
    for t in (0x00, 0x10, 0x01, 0x11):
        bits, vals = HUFF[t]
        body = bytes([t]) + bytes(bits) + bytes.fromhex(vals)
        out += b'\xff\xc4' + (len(body) + 2).to_bytes(2, 'big') + body
    return out + bytes.fromhex('ffda000c' '03' '0100' '0211' '0311' '00' '3f' '00')


def encode(rgb, quality, subsampling='4:4:4', stats=None):
    """uint8 (H, W, 3) -> the whole file."""
    hs, vs = SUBSAMPLING[subsampling]
    h, w, _ = rgb.shape
    coefs = coefficients(rgb, quality, hs, vs)
    return header(h, w, quality, hs, vs) + entropy_code(coefs, h, w, hs, vs, stats) + b'\xff\xd9'


def _upsample(p, hs, vs, ce_h, ce_w):
    """libjpeg's fancy (triangle) up-sampling of a chroma plane over its real extent; plain replication up to 2 columns."""
    p = p[:ce_h, :ce_w].astype(np.int64)
    if hs == 1:
        return p
    if ce_w <= 2:
        return np.repeat(np.repeat(p, vs, axis=0), 2, axis=1)
    if vs == 2:
        up, dn = np.concatenate([p[:1], p[:-1]]), np.concatenate([p[1:], p[-1:]])
        s = np.empty((2 * ce_h, ce_w), np.int64)
        s[0::2], s[1::2] = 3 * p + up, 3 * p + dn
        left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
        out = np.empty((2 * ce_h, 2 * ce_w), np.int64)
        out[:, 0::2], out[:, 1::2] = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
        return out
    left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((ce_h, 2 * ce_w), np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
    return out


def decode_u8(coefs, h, w, quality, hs, vs):
    """Real-block coefficients -> the uint8 (H, W, 3) image libjpeg decodes."""
    planes = []
    for k, c in enumerate(coefs):
        bh, bw, _ = c.shape
        nat = np.zeros((bh, bw, 64), np.int64)
        nat[..., ZZ] = c.astype(np.int64)
        x = idct((nat * qtable(quality, min(k, 1))).reshape(bh, bw, 8, 8))
        p = x.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        if k:
            p = _upsample(p, hs, vs, -(-h // vs), -(-w // hs))
        planes.append(p[:h, :w])
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def to_float(u8):
    return u8.astype(np.float32) / np.float32(255)


def compress(rgb, quality, subsampling='4:4:4'):
    """uint8 (H, W, 3) -> (whole file, decoded uint8 image)."""
    hs, vs = SUBSAMPLING[subsampling]
    h, w, _ = rgb.shape
    coefs = coefficients(rgb, quality, hs, vs)
    data = header(h, w, quality, hs, vs) + entropy_code(coefs, h, w, hs, vs) + b'\xff\xd9'
    return data, decode_u8(coefs, h, w, quality, hs, vs)


# ---- parser: a file's coefficients ------------------------------------------------------------------------------------
def parse(data):
    """A baseline file as written above -> dict(h, w, hs, vs, qtables {id: natural order}, coefs [Y, Cb, Cr] over the whole MCU
    grid (dummy blocks included), ecd_offset)."""
    assert data[:2] == b'\xff\xd8'
    i, q, huff, info = 2, {}, {}, {}
    while True:
        marker, length = data[i:i + 2], int.from_bytes(data[i + 2:i + 4], 'big')
        body = data[i + 4:i + 2 + length]
        if marker == b'\xff\xdb':
            while body:
                q[body[0] & 15] = np.zeros(64, np.int64)
                q[body[0] & 15][ZZ] = list(body[1:65])
                body = body[65:]
        elif marker == b'\xff\xc0':
            info['h'], info['w'] = int.from_bytes(body[1:3], 'big'), int.from_bytes(body[3:5], 'big')
            info['hs'], info['vs'] = body[7] >> 4, body[7] & 15
        elif marker == b'\xff\xc4':
            while body:
                n = sum(body[1:17])
                table, code, k = {}, 0, 17
                for ln in range(1, 17):
                    for _ in range(body[ln]):
                        table[(code, ln)] = body[k]
                        code, k = code + 1, k + 1
                    code <<= 1
                huff[body[0]] = table
                body = body[17 + n:]
        elif marker == b'\xff\xda':
            i += 2 + length
            break
        i += 2 + length
    info['ecd_offset'], info['qtables'] = i, q
    assert data[-2:] == b'\xff\xd9'
    raw = data[i:-2].replace(b'\xff\x00', b'\xff')
    bits = ''.join('{:08b}'.format(b) for b in raw)
    pos = 0

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

    h, w, hs, vs = info['h'], info['w'], info['hs'], info['vs']
    my, mx = -(-h // (8 * vs)), -(-w // (8 * hs))
    coefs = [np.zeros((my * cv, mx * ch, 64), np.int16) for ch, cv in ((hs, vs), (1, 1), (1, 1))]
    pred = [0, 0, 0]
    for r in range(my):
        for c in range(mx):
            for k, (ch, cv) in enumerate(((hs, vs), (1, 1), (1, 1))):
                t = min(k, 1)
                for dy in range(cv):
                    for dx in range(ch):
                        blk = coefs[k][r * cv + dy, c * ch + dx]
                        pred[k] += value(symbol(huff[t]))
                        blk[0] = pred[k]
                        j = 1
                        while j < 64:
                            rs = symbol(huff[0x10 | t])
                            if rs == 0:
                                break
                            j += rs >> 4
                            if rs & 15:
                                blk[j] = value(rs & 15)
                            j += 1
    assert len(bits) - pos < 8 and all(b == '1' for b in bits[pos:])
    info['coefs'] = coefs
    return info
