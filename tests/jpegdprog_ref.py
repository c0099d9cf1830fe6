"""Plain Python restatement of reading progressive JPEG files, next to jpegprog_ref.py: a file taken apart by
its markers alone, the rules and levels of a scan script, a writer for any legal script built on jpegprog_ref's block walks (the test
files of scripts other than libjpeg's come from it), and a model of the decoder as csrc/jpegdprog.h states it - first scans by
speculation, synchronisation rounds, placement and writing over the un-stuffed bit string, DC refine scans a bit per block, AC refine
scans an interval at a time.  Test infrastructure - the product never imports it."""
import numpy as np

import jpeg_ref as ref
import jpegd_ref as dref
import jpegprog_ref as pref

ST_MARKER, ST_CODE, ST_ZIGZAG, ST_CATEGORY, ST_END, ST_BLOCKS, ST_DC, ST_TABLE, ST_OFFSETS, ST_RESTART, ST_RUN = (
    1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)
ALL = (0, 1, 2)

# a script: [(components, Ss, Se, Ah, Al)], the form parse_header's scans begin with
STANDARD = tuple(((ALL if c is None else c), ss, se, ah, al) for c, ss, se, ah, al, _, _ in pref.SCANS)
# spectral selection only
SCRIPT_A = (((0,), 0, 0, 0, 0), ((1,), 0, 0, 0, 0), ((2,), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0))
# three bit planes, the luma band split at its first scan, Cb's last refinement in two bands
SCRIPT_B = ((ALL, 0, 0, 0, 2), ((0,), 1, 2, 0, 0), ((0,), 3, 63, 0, 2), ((1,), 1, 63, 0, 2), ((2,), 1, 63, 0, 2),
            (ALL, 0, 0, 2, 1), ((0,), 3, 63, 2, 1), ((1,), 1, 63, 2, 1), ((2,), 1, 63, 2, 1),
            (ALL, 0, 0, 1, 0), ((0,), 3, 63, 1, 0), ((1,), 1, 10, 1, 0), ((1,), 11, 63, 1, 0), ((2,), 1, 63, 1, 0))
SCRIPTS = {'std': STANDARD, 'A': SCRIPT_A, 'B': SCRIPT_B}


def levels(script):
    """The level of every scan: 1 + the highest level of an earlier scan of a shared component whose band overlaps.  A coefficient
    passes its first scan and one refinement per bit plane, so a script has 1 + (its highest first Al) levels at the most."""
    out = []
    for cs, ss, se, _, _ in script:
        out.append(1 + max([lv for lv, (ce, es, ee, _, _) in zip(out, script) if set(ce) & set(cs) and es <= se and ss <= ee] or [0]))
    return out


def legal(script):
    """T.81 G.1.1.1 as the product reads it, completeness included."""
    al_of = [[None] * 64 for _ in range(3)]
    if not 1 <= len(script) <= 64:
        return False
    for cs, ss, se, ah, al in script:
        if tuple(cs) not in ((0,), (1,), (2,), ALL) or not 0 <= ss <= se <= 63 or (ss == 0 and se != 0) or (ss > 0 and len(cs) != 1):
            return False
        if not (0 <= ah <= 13 and 0 <= al <= 13):
            return False
        for c in cs:
            if ss > 0 and al_of[c][0] is None:
                return False
            for k in range(ss, se + 1):
                if (al_of[c][k] is not None) if ah == 0 else (al_of[c][k] != ah or al != ah - 1):
                    return False
                al_of[c][k] = al
    return all(v == 0 for row in al_of for v in row)


def mask_rows(script):
    """(n_scans, 6) int32 as nimg_jpeg_decode_progressive takes a script: component mask, Ss, Se, Ah, Al, level."""
    return np.array([[sum(1 << c for c in cs), ss, se, ah, al, lv] for (cs, ss, se, ah, al), lv in zip(script, levels(script))],
                    np.int32).reshape(-1, 6)


# ---- a writer for any script ------------------------------------------------------------------------------------------------
def _sos(cs, ss, se, ah, al):
    # DC first scans take DC table 0 for Y and 1 for chroma; an AC scan's table is written in front of it under the same ids; a DC
    # refine scan names none (libjpeg writes 0)
    body = bytes([len(cs)]) + b''.join(bytes([c + 1, (0x11 if c else 0x00) & (0x0f if ss else (0x00 if ah else 0xf0))]) for c in cs)
    body += bytes([ss, se, (ah << 4) | al])
    return b'\xff\xda' + (len(body) + 2).to_bytes(2, 'big') + body


def encode(coefs, h, w, hs, vs, prefix, script, restart_interval=0):
    """One image's coefficients -> the whole file of `script`, every table the optimal one of its scan (the two DC tables: of all
    DC first scans).  jpegprog_ref's walks, which read the script from the module's SCANS."""
    rows, t = [], 2
    for cs, ss, se, ah, al in script:
        table = None
        if ss > 0:
            table, t = t, t + 1
        rows.append((None if tuple(cs) == ALL else tuple(cs), ss, se, ah, al, None, table))
    saved = pref.SCANS
    pref.SCANS = tuple(rows)
    try:
        items = [pref.scan_items(coefs, h, w, hs, vs, i, restart_interval) for i in range(len(rows))]
    finally:
        pref.SCANS = saved
    hist = np.zeros((t, 257), np.uint32)
    for scan in items:
        for it in scan:
            if it[0] == 'sym':
                hist[it[1], it[2]] += 1
    tables, status = pref.opt.optimal_tables(hist)
    assert not status.any()
    out = prefix + pref.dht(0x00, tables[0]) + pref.dht(0x01, tables[1])
    if restart_interval:
        out += b'\xff\xdd\x00\x04' + int(restart_interval).to_bytes(2, 'big')
    for row, (cs, ss, se, ah, al), scan in zip(rows, script, items):
        seg, st = pref.code_segment(scan, tables)
        assert st == 0
        if row[6] is not None:
            out += pref.dht(0x11 if cs[0] else 0x10, tables[row[6]])
        out += _sos(cs, ss, se, ah, al) + seg
    return out + b'\xff\xd9'


# ---- a file by its markers ----------------------------------------------------------------------------------------------------
def split(data):
    """dict(h, w, hs, vs, ri, q = [table id per component], qtables, script, tables = per scan [(counts, symbols) per component of
    the scan, (16 zeros, b'') where it has none], segments = per scan the stuffed bytes with their restart markers)."""
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
        elif marker == 0xc2:
            out['h'], out['w'] = int.from_bytes(body[1:3], 'big'), int.from_bytes(body[3:5], 'big')
            out['hs'], out['vs'] = body[7] >> 4, body[7] & 15
            out['q'] = [body[8 + 3 * c] for c in range(3)]
        elif marker == 0xc4:
            while body:
                n = sum(body[1:17])
                dht[body[0]] = (bytes(body[1:17]), bytes(body[17:17 + n]))
                body = body[17 + n:]
        elif marker == 0xdd:
            out['ri'] = int.from_bytes(body, 'big')
        elif marker == 0xda:
            ns = body[0]
            cs = tuple(body[1 + 2 * c] - 1 for c in range(ns))
            ss, se, ah, al = body[1 + 2 * ns], body[2 + 2 * ns], body[3 + 2 * ns] >> 4, body[3 + 2 * ns] & 15
            out['script'].append((cs, ss, se, ah, al))
            sel = [body[2 + 2 * c] for c in range(ns)]
            out['tables'].append([(bytes(16), b'') if ss == 0 and ah else dht[(s >> 4) if ss == 0 else 0x10 | (s & 15)] for s in sel])
            j = i
            while not (data[j] == 0xff and data[j + 1] != 0 and not 0xd0 <= data[j + 1] <= 0xd7):
                j += 1
            out['segments'].append(data[i:j])
            i = j
    out['qtables'] = q
    return out


def table_bytes(tables):
    """[(counts, symbols)] of one scan -> (3, 272) uint8, slot c = the table of the scan's c-th component."""
    out = np.zeros((3, 272), np.uint8)
    for t, (counts, symbols) in enumerate(tables):
        out[t, :16] = list(counts)
        out[t, 16:16 + len(symbols)] = list(symbols)
    return out


# ---- the model of the decoder ---------------------------------------------------------------------------------------------------
class Geometry(object):
    def __init__(self, h, w, hs, vs, ri):
        comps, (my, mx) = ref.geometry(h, w, hs, vs)
        self.hs, self.vs, self.mx, self.my, self.per, self.ri = hs, vs, mx, my, hs * vs + 2, ri
        self.shapes = [(c[2], c[3]) for c in comps]
        self.base = np.concatenate([[0], np.cumsum([r * c for r, c in self.shapes])]).tolist()
        self.SB = my * mx * self.per

    def scan(self, cs):
        """(blocks of the scan, blocks per MCU, blocks per restart interval, intervals)"""
        blocks, per = (self.SB, self.per) if len(cs) == 3 else (self.shapes[cs[0]][0] * self.shapes[cs[0]][1], 1)
        span = self.ri * per if self.ri else blocks
        return blocks, per, span, -(-blocks // span)

    def place(self, cs, b):
        """block b of a scan -> (component, offset in blocks in the device tensor or -1 for a dummy)"""
        if len(cs) == 1:
            return cs[0], self.base[cs[0]] + b
        mcu, k = divmod(b, self.per)
        ny = self.per - 2
        if k >= ny:
            return k - ny + 1, self.base[k - ny + 1] + mcu
        br, bc = (mcu // self.mx) * self.vs + k // self.hs, (mcu % self.mx) * self.hs + k % self.hs
        return 0, (br * self.shapes[0][1] + bc if br < self.shapes[0][0] and bc < self.shapes[0][1] else -1)


def unstuff(ecd, rst, K):
    """-> (bit string, the bit every interval begins at [K + 1], status)"""
    at = lambda k: ecd[k] if 0 <= k < len(ecd) else 1
    kept, ibit, status, met = bytearray(), [0] * (K + 1), 0, 0
    for k, b in enumerate(ecd):
        if rst and b == 0xff and (at(k + 1) & 0xf8) == 0xd0:
            if met + 1 >= K:
                status |= ST_RESTART
            else:
                ibit[met + 1] = 8 * len(kept)
                status |= 0 if (at(k + 1) & 7) == (met & 7) else ST_RESTART
            met += 1
            continue
        if rst and at(k - 1) == 0xff and (b & 0xf8) == 0xd0:
            continue
        if b == 0xff and at(k + 1) != 0:
            status |= ST_MARKER
        if b == 0 and at(k - 1) == 0xff:
            continue
        kept.append(b)
    total = 8 * len(kept)
    if rst and met + 1 != K:
        status |= ST_RESTART
    for k in range(min(met, K - 1) + 1, K + 1):
        ibit[k] = total
    return ''.join('{:08b}'.format(b) for b in kept), ibit, status


def _extend(v, sz):
    return v if sz == 0 or v >> (sz - 1) else v - (1 << sz) + 1


class Scan(object):
    """One scan of one image over the image's flat coefficients (int64, updated in place)."""

    def __init__(self, geo, scan, tables, ecd, coef):
        self.geo, (self.cs, self.ss, self.se, self.ah, self.al), self.coef = geo, scan, coef
        self.blocks, self.per, self.span, self.K = geo.scan(self.cs)
        self.luts = dref._lookups([t for t in tables])
        self.status = 0
        for counts, symbols in tables:
            code = 0
            for ln in range(1, 17):
                code += counts[ln - 1]
                if code > (1 << ln):
                    self.status |= ST_TABLE
                code <<= 1
        self.bits, self.ibit, st = unstuff(ecd, geo.ri != 0, self.K)
        self.status |= st
        self.total = len(self.bits)
        self.big = int(self.bits + '0' * 32, 2) if self.bits else 0

    def window(self, p):
        return (self.big >> (self.total - p)) & 0xffffffff if p <= self.total else 0

    def symbol(self, slot, p):
        e = self.luts[slot][self.window(p) >> 16]
        return (e >> 8, e & 255) if e else (0, -1)

    def first(self, state, limit, end, write=None):
        """One subsequence of a first scan from `state` = (p, m, k) or None.  write = (first block completed here, interval's first
        block, its end, dcdiff).  -> (exit state, blocks completed)"""
        if state is None:
            return None, 0
        p, m, k = state
        done, ny, dc = 0, self.per - 2, self.ss == 0
        if write:
            cur, b0, b1, dcdiff = write
            if cur < b0 or cur > b1:
                return state, 0
        fail = 0
        while p < limit:
            if write and cur >= b1:
                break
            ln, sym = self.symbol((m - ny + 1 if dc and self.per > 1 and m >= ny else 0), p)
            if sym < 0:
                fail = ST_CODE
                break
            w = self.window(p)
            if dc:
                if sym > 11:
                    fail = ST_CATEGORY
                    break
                if p + ln + sym > end:
                    fail = ST_END
                    break
                if write:
                    dcdiff[cur] = _extend((w >> (32 - ln - sym)) & ((1 << sym) - 1), sym)
                p, m, done = p + ln + sym, (m + 1) % self.per, done + 1
                cur = cur + 1 if write else 0
                continue
            sz, r = sym & 15, sym >> 4
            if sz > 10:
                fail = ST_CATEGORY
                break
            if sz == 0 and r < 15:
                if p + ln + r > end:
                    fail = ST_END
                    break
                run = (1 << r) + ((w >> (32 - ln - r)) & ((1 << r) - 1))
                if write and run > b1 - cur:
                    fail = ST_RUN
                    break
                p, done, k = p + ln + r, done + run, self.ss
                cur = cur + run if write else 0
            elif sz == 0:
                if p + ln > end:
                    fail = ST_END
                    break
                p, k = p + ln, k + 16
                if k > self.se:
                    k, done = self.ss, done + 1
                    cur = cur + 1 if write else 0
            else:
                if p + ln + sz > end:
                    fail = ST_END
                    break
                k += r
                if k > self.se:
                    fail = ST_ZIGZAG
                    break
                if write:
                    at = self.geo.place(self.cs, cur)[1]
                    if at >= 0:
                        self.coef[at * 64 + k] = _extend((w >> (32 - ln - sz)) & ((1 << sz) - 1), sz) << self.al
                p, k = p + ln + sz, k + 1
                if k > self.se:
                    k, done = self.ss, done + 1
                    cur = cur + 1 if write else 0
        if fail:
            if write:
                self.status |= fail
            return None, done
        return (p, m, k), done

    def run_first(self, subseq_bits):
        """-> rounds"""
        sb = subseq_bits or max(32, -(-self.total // 32) * 32)
        spans = []                       # per subsequence: (interval, index in it, start, limit, end)
        for j in range(self.K):
            lo, hi = self.ibit[j], self.ibit[j + 1]
            for i in range(max(1, -(-(hi - lo) // sb))):
                spans.append((j, i, lo + i * sb, min(lo + (i + 1) * sb, hi), hi))
        longest = max(sum(1 for s in spans if s[0] == j) for j in range(self.K))
        done = [self.first((s[2], 0, self.ss), s[3], s[4]) for s in spans]
        rounds = 0
        while rounds + 1 < longest:
            rounds += 1
            new = [self.first(done[i - 1][0], s[3], s[4]) if i >= rounds and s[1] >= rounds else done[i] for i, s in enumerate(spans)]
            changed = any(a[0] != b[0] for a, b in zip(new, done))
            done = new
            if not changed:
                break
        first = np.concatenate([[0], np.cumsum([d[1] for d in done])]).tolist()
        start = [next(i for i, s in enumerate(spans) if s[0] == j) for j in range(self.K)] + [len(spans)]
        for j in range(self.K):
            if (first[start[j + 1]] - first[start[j]]) & 0xffffffff < min(self.span, self.blocks - j * self.span):
                self.status |= ST_BLOCKS
        dcdiff = [0] * self.blocks
        for i, s in enumerate(spans):
            b0 = s[0] * self.span
            state = done[i - 1][0] if s[1] else (s[2], 0, self.ss)
            self.first(state, s[3], s[4], (b0 + first[i] - first[start[s[0]]], b0, min(b0 + self.span, self.blocks), dcdiff))
        if self.ss == 0:
            pred = [0, 0, 0]
            for b in range(self.blocks):
                comp, at = self.geo.place(self.cs, b)
                if b % self.span == 0:
                    pred = [0, 0, 0]
                pred[comp] += dcdiff[b]
                v = pred[comp] << self.al
                if not -32768 <= v <= 32767:
                    self.status |= ST_DC
                if at >= 0:
                    self.coef[at * 64] = v
        return rounds

    def run_dc_refine(self):
        for b in range(self.blocks):
            j = b // self.span
            pos = self.ibit[j] + b - j * self.span
            if pos >= self.ibit[j + 1]:
                self.status |= ST_END
                continue
            at = self.geo.place(self.cs, b)[1]
            if at >= 0 and self.bits[pos] == '1':
                self.coef[at * 64] |= 1 << self.al

    def _correct(self, at, p):
        c = int(self.coef[at])
        if self.bits[p] == '1' and (c & (1 << self.al)) == 0:
            self.coef[at] = c + (1 << self.al) if c >= 0 else c - (1 << self.al)

    def _ac_refine(self, p, end, at0, nblocks):
        """libjpeg's decode_mcu_AC_refine over one interval -> status"""
        p1, eobrun = 1 << self.al, 0
        for b in range(nblocks):
            at, k = (at0 + b) * 64, self.ss
            if eobrun == 0:
                while k <= self.se:
                    ln, sym = self.symbol(0, p)
                    if sym < 0:
                        return ST_CODE
                    w, sz, r, fresh = self.window(p), sym & 15, sym >> 4, 0
                    if sz:
                        if sz != 1:
                            return ST_CATEGORY
                        if p + ln + 1 > end:
                            return ST_END
                        fresh = p1 if (w >> (31 - ln)) & 1 else -p1
                        p += ln + 1
                    elif r != 15:
                        if p + ln + r > end:
                            return ST_END
                        run = (1 << r) + ((w >> (32 - ln - r)) & ((1 << r) - 1))
                        if run > nblocks - b:
                            return ST_RUN
                        p, eobrun = p + ln + r, run
                        break
                    else:
                        if p + ln > end:
                            return ST_END
                        p += ln
                    while k <= self.se:
                        if self.coef[at + k] != 0:
                            if p >= end:
                                return ST_END
                            self._correct(at + k, p)
                            p += 1
                        else:
                            r -= 1
                            if r < 0:
                                break
                        k += 1
                    if fresh:
                        if k > self.se:
                            return ST_ZIGZAG
                        self.coef[at + k] = fresh
                    k += 1
            if eobrun > 0:
                while k <= self.se:
                    if self.coef[at + k] != 0:
                        if p >= end:
                            return ST_END
                        self._correct(at + k, p)
                        p += 1
                    k += 1
                eobrun -= 1
        return 0

    def run_ac_refine(self):
        for j in range(self.K):
            b0 = j * self.span
            self.status |= self._ac_refine(self.ibit[j], self.ibit[j + 1], self.geo.base[self.cs[0]] + b0, min(self.span, self.blocks - b0))


def decode_scans(h, w, hs, vs, ri, script, tables, segments, subseq_bits=0):
    """-> (flat int16 coefficients in the device layout, status, [rounds per scan]); the scans level after level, as the device
    orders them."""
    geo = Geometry(h, w, hs, vs, ri)
    coef = np.zeros(geo.base[3] * 64, np.int64)
    lv = levels(script)
    status, rounds = 0, [0] * len(script)
    for level in range(1, max(lv) + 1):
        for s, scan in enumerate(script):
            if lv[s] != level:
                continue
            model = Scan(geo, scan, tables[s], segments[s], coef)
            if scan[3] == 0:
                rounds[s] = model.run_first(subseq_bits)
            elif scan[1] == 0:
                model.run_dc_refine()
            else:
                model.run_ac_refine()
            status |= model.status
    return coef.astype(np.int16), status, rounds


def decode(data, subseq_bits=0):
    """A progressive file -> (flat coefficients, status, [rounds per scan])."""
    p = split(data)
    assert legal(p['script'])
    return decode_scans(p['h'], p['w'], p['hs'], p['vs'], p['ri'], p['script'], p['tables'], p['segments'], subseq_bits)


def decode_u8(data):
    """The image libjpeg decodes from a complete progressive file: the model's coefficients through jpeg_ref's inverse transform."""
    p = split(data)
    flat, status, _ = decode(data)
    assert status == 0
    geo = Geometry(p['h'], p['w'], p['hs'], p['vs'], p['ri'])
    h, w, hs, vs = p['h'], p['w'], p['hs'], p['vs']
    planes = []
    for k, (bh, bw) in enumerate(geo.shapes):
        c = flat[geo.base[k] * 64:geo.base[k + 1] * 64].reshape(bh, bw, 64).astype(np.int64)
        nat = np.zeros((bh, bw, 64), np.int64)
        nat[..., ref.ZZ] = c
        x = ref.idct((nat * p['qtables'][p['q'][k]]).reshape(bh, bw, 8, 8))
        pl = x.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        if k:
            pl = ref._upsample(pl, hs, vs, -(-h // vs), -(-w // hs))
        planes.append(pl[:h, :w])
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
