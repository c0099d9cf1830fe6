"""Plain Python restatement of the JPEG decoder of DESIGN.md section 4e, next to jpeg_ref.py: the header of a file with its
Huffman tables, the decode of jpeg_ref.parse's coefficients with the tables parsed from the file, and a model of the parallel
algorithm (speculate, synchronise, place, write, DC) over the un-stuffed bit string.  Test infrastructure - the product never
imports it."""
import numpy as np

import jpeg_ref as ref

ST_MARKER, ST_CODE, ST_ZIGZAG, ST_CATEGORY, ST_END, ST_BLOCKS, ST_DC = 1, 2, 4, 8, 16, 32, 64


def header(data):
    """dict(h, w, hs, vs, q = [table id per component], tables = [(counts, symbols)] x 6 in the order Y-DC, Y-AC, Cb-DC, Cb-AC,
    Cr-DC, Cr-AC, qtables {id: natural order}, ecd_offset, ecd_end) of a baseline file with one scan that ends with EOI."""
    assert data[:2] == b'\xff\xd8' and data[-2:] == b'\xff\xd9'
    i, q, dht, out = 2, {}, {}, {}
    while True:
        marker, length = data[i + 1], int.from_bytes(data[i + 2:i + 4], 'big')
        body = data[i + 4:i + 2 + length]
        if marker == 0xdb:
            while body:
                q[body[0] & 15] = np.zeros(64, np.int64)
                q[body[0] & 15][ref.ZZ] = list(body[1:65])
                body = body[65:]
        elif marker == 0xc0:
            out['h'], out['w'] = int.from_bytes(body[1:3], 'big'), int.from_bytes(body[3:5], 'big')
            out['hs'], out['vs'] = body[7] >> 4, body[7] & 15
            out['q'] = [body[8 + 3 * c] for c in range(3)]
        elif marker == 0xc4:
            while body:
                n = sum(body[1:17])
                dht[body[0]] = (bytes(body[1:17]), bytes(body[17:17 + n]))
                body = body[17 + n:]
        elif marker == 0xda:
            out['tables'] = [dht[cls << 4 | ((body[2 + 2 * c] >> 4) if cls == 0 else (body[2 + 2 * c] & 15))]
                             for c in range(3) for cls in (0, 1)]
            i += 2 + length
            break
        i += 2 + length
    out['qtables'], out['ecd_offset'], out['ecd_end'] = q, i, len(data) - 2
    return out


def huffman_bytes(head):
    """The six tables as nimg_jpeg_decode takes them: (6, 272) uint8, 16 counts then the symbols."""
    out = np.zeros((6, 272), np.uint8)
    for t, (counts, symbols) in enumerate(head['tables']):
        out[t, :16] = list(counts)
        out[t, 16:16 + len(symbols)] = list(symbols)
    return out


def real_coefficients(info):
    """jpeg_ref.parse's coefficients (whole MCU grid) -> [Y, Cb, Cr] over the real blocks."""
    comps, _ = ref.geometry(info['h'], info['w'], info['hs'], info['vs'])
    return [c[:comps[k][2], :comps[k][3]] for k, c in enumerate(info['coefs'])]


def decode_u8(data):
    """The image libjpeg decodes from a file: jpeg_ref.parse's coefficients, the tables of the file, jpeg_ref's inverse transform."""
    info, head = ref.parse(data), header(data)
    h, w, hs, vs = info['h'], info['w'], info['hs'], info['vs']
    planes = []
    for k, c in enumerate(real_coefficients(info)):
        bh, bw, _ = c.shape
        nat = np.zeros((bh, bw, 64), np.int64)
        nat[..., ref.ZZ] = c.astype(np.int64)
        x = ref.idct((nat * info['qtables'][head['q'][k]]).reshape(bh, bw, 8, 8))
        p = x.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        if k:
            p = ref._upsample(p, hs, vs, -(-h // vs), -(-w // hs))
        planes.append(p[:h, :w])
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


# ---- the model of the parallel algorithm ------------------------------------------------------------------------------------
def _lookup(counts, symbols):
    """The next 16 bits -> length << 8 | symbol, 0 where no code starts."""
    lut, code, k = [0] * 65536, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            lo = code << (16 - ln)
            lut[lo:lo + (1 << (16 - ln))] = [ln << 8 | symbols[k]] * (1 << (16 - ln))
            code, k = code + 1, k + 1
        code <<= 1
    return lut


_LOOKUPS = {}


def _lookups(tables):
    for t in tables:
        if t not in _LOOKUPS:
            _LOOKUPS[t] = _lookup(*t)
    return [_LOOKUPS[t] for t in tables]


class Model(object):
    """Steps 1 to 6 over one image: model = Model(h, w, hs, vs, tables, ecd); model.run(subseq_bits) -> (flat coefficients in the
    device layout, status, rounds, subsequences).  subseq_bits 0 = one subsequence as long as the stream."""

    def __init__(self, h, w, hs, vs, tables, ecd):
        comps, (my, mx) = ref.geometry(h, w, hs, vs)
        self.hs, self.vs, self.mx, self.per = hs, vs, mx, hs * vs + 2
        self.shapes = [(c[2], c[3]) for c in comps]
        self.base = np.concatenate([[0], np.cumsum([r * c for r, c in self.shapes])]).tolist()
        self.SB = my * mx * self.per
        self.luts = _lookups(tables)
        self.status = ST_MARKER if any(b == 0xff and (k + 1 >= len(ecd) or ecd[k + 1] != 0) for k, b in enumerate(ecd)) else 0
        raw = bytes(b for k, b in enumerate(ecd) if not (b == 0 and k > 0 and ecd[k - 1] == 0xff))
        self.bits = ''.join('{:08b}'.format(b) for b in raw)                    # jpeg_ref's bit string
        self.total = len(self.bits)
        self.big = int(self.bits + '0' * 32, 2)

    def place(self, b):
        """scan-order block -> (component, offset in blocks in the device tensor or -1 for a dummy)."""
        mcu, k = divmod(b, self.per)
        ny = self.per - 2
        if k >= ny:
            return k - ny + 1, self.base[k - ny + 1] + mcu
        br, bc = (mcu // self.mx) * self.vs + k // self.hs, (mcu % self.mx) * self.hs + k % self.hs
        return 0, (br * self.shapes[0][1] + bc if br < self.shapes[0][0] and bc < self.shapes[0][1] else -1)

    def decode(self, state, limit, write=None):
        """One subsequence from `state` = (p, m, z) or None (invalid).  write = (first block begun here, coef, dcdiff) stores and
        sets status bits.  Returns (exit state, blocks begun)."""
        if state is None:
            return None, 0
        p, m, z = state
        begun, ny = 0, self.per - 2
        if write:
            cur, coef, dcdiff = write[0] - (1 if z else 0), write[1], write[2]
            at = -1
            if z:
                if write[0] == 0 or cur >= self.SB:
                    return state, 0
                at = self.place(cur)[1]
        while p < limit:
            if write and z == 0 and cur >= self.SB:
                break
            c = 0 if m < ny else m - ny + 1
            window = (self.big >> (self.total - p)) & 0xffffffff
            e = self.luts[2 * c + (1 if z else 0)][window >> 16]
            fail = 0
            if e == 0:
                fail = ST_CODE
            else:
                ln, sym = e >> 8, e & 255
                sz, run = (sym & 15, sym >> 4) if z else (sym, 0)
                if sz > (10 if z else 11):
                    fail = ST_CATEGORY
                elif p + ln + sz > self.total:
                    fail = ST_END
            if fail:
                if write:
                    self.status |= fail
                return None, begun
            v = 0
            if sz:
                v = (window >> (32 - ln - sz)) & ((1 << sz) - 1)
                v = v if v >> (sz - 1) else v - (1 << sz) + 1
            p += ln + sz
            end = False
            if z == 0:
                begun += 1
                if write:
                    dcdiff[cur] = v
                    at = self.place(cur)[1]
                z = 1
            elif sz == 0:
                z += 16
                end = run != 15 or z > 63
            else:
                z += run
                if z > 63:
                    if write:
                        self.status |= ST_ZIGZAG
                    end = True
                else:
                    if write and at >= 0:
                        coef[at * 64 + z] = v
                    z += 1
                    end = z == 64
            if end:
                z, m = 0, (m + 1) % self.per
                if write:
                    cur, at = cur + 1, -1
        return (p, m, z), begun

    def run(self, subseq_bits):
        sb = subseq_bits or max(32, -(-self.total // 32) * 32)
        S = max(1, -(-self.total // sb))
        limit = [min((i + 1) * sb, self.total) for i in range(S)]
        status0, self.status = self.status, self.status
        done = [self.decode((i * sb, 0, 0), limit[i]) for i in range(S)]                     # speculate
        rounds = 0
        while rounds + 1 < S:                                                                 # synchronise
            rounds += 1
            new = done[:rounds] + [self.decode(done[i - 1][0], limit[i]) for i in range(rounds, S)]
            changed = any(a[0] != b[0] for a, b in zip(new, done))
            done = new
            if not changed:
                break
        first = np.concatenate([[0], np.cumsum([d[1] for d in done])]).tolist()             # place
        if first[-1] < self.SB:
            self.status |= ST_BLOCKS
        coef, dcdiff = np.zeros(self.base[3] * 64, np.int64), [0] * self.SB
        for i in range(S):                                                                    # write
            self.decode(done[i - 1][0] if i else (0, 0, 0), limit[i], (first[i], coef, dcdiff))
        pred = [0, 0, 0]
        for b in range(self.SB):                                                              # DC, through the dummy blocks
            comp, at = self.place(b)
            pred[comp] += dcdiff[b]
            if not -32768 <= pred[comp] <= 32767:
                self.status |= ST_DC
            if at >= 0:
                coef[at * 64] = pred[comp]
        status, self.status = self.status, status0
        return coef.astype(np.int16), status, rounds, S
