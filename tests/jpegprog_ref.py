"""Plain Python restatement of progressive JPEG files (what libjpeg writes with jpeg_simple_progression, Pillow's
progressive=True): the ten scans of the script, the four block walks of T.81 Annex G with libjpeg's choices, the end-of-band runs
with their forced flushes, the symbol histograms, and the file with its DHT and SOS segments between the scans.  Built on jpeg_ref.py
and jpegopt_ref.py, test infrastructure like them - the product never imports it.  The ten tables of an image stand in the order the
file's DHT segments have: DC 00, DC 01, then the AC tables of the scans 2, 3, 4, 5, 6, 8, 9, 10 (1-based)."""
import numpy as np

import jpeg_ref as ref
import jpegopt_ref as opt

# (components or None = all three interleaved, Ss, Se, Ah, Al, DHT id of the AC table or None, index among the ten tables)
SCANS = ((None, 0, 0, 0, 1, None, 0), ((0,), 1, 5, 0, 2, 0x10, 2), ((2,), 1, 63, 0, 1, 0x11, 3), ((1,), 1, 63, 0, 1, 0x11, 4),
         ((0,), 6, 63, 0, 2, 0x10, 5), ((0,), 1, 63, 2, 1, 0x10, 6), (None, 0, 0, 1, 0, None, None), ((2,), 1, 63, 1, 0, 0x11, 7),
         ((1,), 1, 63, 1, 0, 0x11, 8), ((0,), 1, 63, 1, 0, 0x10, 9))
N_SCANS, N_TABLES = 10, 10
TABLE_IDS = (0x00, 0x01, 0x10, 0x11, 0x11, 0x10, 0x10, 0x11, 0x11, 0x10)
BE_FLUSH = 937                       # libjpeg flushes a run once more than MAX_CORR_BITS - DCTSIZE2 + 1 correction bits wait
COUNTERS = ('zrl_first', 'zrl_refine', 'refine_tail_run', 'eobrun_cat0', 'eobrun_cat1', 'eobrun_cat5plus', 'flush_7fff', 'flush_937',
            'dummy_right', 'dummy_bottom', 'restart_in_run', 'pad_some', 'pad_none')


def clamp_dc(v):
    return min(max(int(v), -2047), 2047)


def clamp_ac(v):
    return min(max(int(v), -1023), 1023)


class _Scan(object):
    """One scan's output as items: ('sym', table, symbol, value, nbits) | ('bits', value, nbits) | ('rst', k), and its run state."""

    def __init__(self, table, stats):
        self.items, self.table, self.stats = [], table, stats
        self.eobrun, self.be = 0, []

    def symbol(self, table, sym, value=0, nbits=0):
        self.items.append(('sym', table, sym, value & ((1 << nbits) - 1), nbits))

    def bits(self, bits):
        for b in bits:
            self.items.append(('bits', b, 1))

    def emit_eobrun(self):
        if self.eobrun > 0:
            n = self.eobrun.bit_length() - 1
            self.stats['eobrun_cat0'] += n == 0
            self.stats['eobrun_cat1'] += n == 1
            self.stats['eobrun_cat5plus'] += n >= 5
            self.symbol(self.table, n << 4, self.eobrun, n)
            self.bits(self.be)
            self.eobrun, self.be = 0, []


def _ac_first(s, blk, ss, se, al):
    r = 0
    for k in range(ss, se + 1):
        v = clamp_ac(blk[k])
        t = abs(v) >> al
        if t == 0:
            r += 1
            continue
        s.emit_eobrun()
        while r > 15:
            s.symbol(s.table, 0xf0)
            s.stats['zrl_first'] += 1
            r -= 16
        nb = t.bit_length()
        s.symbol(s.table, (r << 4) + nb, t if v > 0 else ~t, nb)
        r = 0
    if r > 0:
        s.eobrun += 1
        if s.eobrun == 0x7fff:
            s.stats['flush_7fff'] += 1
            s.emit_eobrun()


def _ac_refine(s, blk, ss, se, al):
    a = [abs(clamp_ac(v)) >> al for v in blk]
    eob = max([k for k in range(ss, se + 1) if a[k] == 1] or [0])
    r, br = 0, []
    for k in range(ss, se + 1):
        if a[k] == 0:
            r += 1
            continue
        while r > 15 and k <= eob:
            s.emit_eobrun()
            s.symbol(s.table, 0xf0)
            s.stats['zrl_refine'] += 1
            r -= 16
            s.bits(br)
            br = []
        if a[k] > 1:
            s.stats['refine_tail_run'] += r > 15             # behind the last new coefficient: the zeros stay in the run
            br.append(a[k] & 1)
            continue
        s.emit_eobrun()
        s.symbol(s.table, (r << 4) + 1, 1 if blk[k] > 0 else 0, 1)
        s.bits(br)
        br, r = [], 0
    if r > 0 or br:
        s.eobrun += 1
        s.be += br
        if s.eobrun == 0x7fff or len(s.be) > BE_FLUSH:
            s.stats['flush_7fff' if s.eobrun == 0x7fff else 'flush_937'] += 1
            s.emit_eobrun()


def scan_items(coefs, h, w, hs, vs, index, restart_interval=0, stats=None):
    """The items of scan `index` (0..9) of one image; coefs as jpeg_ref.coefficients gives them."""
    stats = stats if stats is not None else {}
    for key in COUNTERS:
        stats.setdefault(key, 0)
    comps, ss, se, ah, al, _, table = SCANS[index]
    s = _Scan(table, stats)
    if comps is None:
        per = hs * vs + 2
        blocks = [(k, blk, kind) for k, blk, kind in ref.scan_blocks(coefs, h, w, hs, vs)]
    else:
        per = 1
        blocks = [(comps[0], blk, None) for blk in coefs[comps[0]].reshape(-1, 64)]
        empty = ~coefs[comps[0]].reshape(-1, 64)[:, ss:se + 1].any(axis=1)
    pred, markers = [0, 0, 0], 0
    for j, (k, blk, kind) in enumerate(blocks):
        if restart_interval and j and j % (restart_interval * per) == 0:
            stats['restart_in_run'] += s.eobrun > 0
            s.emit_eobrun()
            s.items.append(('rst', markers & 7))
            markers += 1
            pred = [0, 0, 0]
        if kind:
            stats['dummy_' + kind] += 1
        if ss > 0 and empty[j]:                     # an empty band in either kind of AC scan: the block only joins the run
            s.eobrun += 1
            if s.eobrun == 0x7fff:
                stats['flush_7fff'] += 1
                s.emit_eobrun()
        elif ss == 0 and ah == 0:
            v = clamp_dc(blk[0]) >> al
            d = v - pred[k]
            pred[k] = v
            nb = ref._category(d)
            s.symbol(min(k, 1), nb, d if d >= 0 else d - 1, nb)
        elif ss == 0:
            s.bits([(clamp_dc(blk[0]) >> al) & 1])
        elif ah == 0:
            _ac_first(s, blk.tolist(), ss, se, al)
        else:
            _ac_refine(s, blk.tolist(), ss, se, al)
    s.emit_eobrun()
    return s.items


def all_items(coefs, h, w, hs, vs, restart_interval=0, stats=None):
    return [scan_items(coefs, h, w, hs, vs, i, restart_interval, stats) for i in range(N_SCANS)]


def histograms(items):
    """(10, 257) uint32 - what nimg_jpeg_progressive_histogram writes for one image."""
    hist = np.zeros((N_TABLES, 257), np.uint32)
    for scan in items:
        for it in scan:
            if it[0] == 'sym':
                hist[it[1], it[2]] += 1
    return hist


def code_segment(items, tables, stats=None):
    """One scan's items with the ten tables (10, 272) -> (stuffed bytes with the restart markers, status)."""
    bits, out, status, codes = ref._Bits(), b'', 0, {}

    def pad():
        if stats is not None:
            stats['pad_some' if bits.n else 'pad_none'] += 1
        if bits.n:
            bits.put(0xff, 8 - bits.n)
        return bytes(bits.out).replace(b'\xff', b'\xff\x00')

    for it in items:
        if it[0] == 'sym':
            if it[1] not in codes:
                codes[it[1]] = opt.codes_of(tables[it[1]], it[1] < 2)[0]
            if it[2] not in codes[it[1]]:
                status |= opt.ST_SYMBOL
                continue
            bits.put(*codes[it[1]][it[2]])
            bits.put(it[3], it[4])
        elif it[0] == 'bits':
            bits.put(it[1], it[2])
        else:
            out += pad() + bytes([0xff, 0xd0 + it[1]])
            bits = ref._Bits()
    return out + pad(), status


def segments(items, tables, stats=None):
    """-> ([10 segments], status) as nimg_jpeg_encode_progressive; tables that are no prefix code leave the restart markers alone."""
    if not all(opt.codes_of(t, i < 2)[1] for i, t in enumerate(tables)):
        return [b''.join(bytes([0xff, 0xd0 + it[1]]) for it in scan if it[0] == 'rst') for scan in items], opt.ST_TABLE
    done = [code_segment(it, tables, stats) for it in items]
    status = 0
    for _, st in done:
        status |= st
    return [d[0] for d in done], status


def dht(ident, table):
    n = int(np.sum(table[:16], dtype=np.int64))
    return b'\xff\xc4' + (19 + n).to_bytes(2, 'big') + bytes([ident]) + bytes(np.asarray(table[:16 + n]).tolist())


def sos(index):
    comps, ss, se, ah, al, ident, _ = SCANS[index]
    if comps is None:
        body = bytes([3, 1, 0x00, 2, 0x10 if ss == 0 and ah == 0 else 0x00, 3, 0x10 if ss == 0 and ah == 0 else 0x00])
    else:
        body = bytes([1, comps[0] + 1, ident & 1])
    body += bytes([ss, se, (ah << 4) | al])
    return b'\xff\xda' + (len(body) + 2).to_bytes(2, 'big') + body


def assemble(prefix, segs, tables, restart_interval=0):
    """prefix: SOI .. the end of the frame header (SOF2 already in it) -> the whole file."""
    out = prefix + dht(0x00, tables[0]) + dht(0x01, tables[1])
    if restart_interval:
        out += b'\xff\xdd\x00\x04' + int(restart_interval).to_bytes(2, 'big')
    for i in range(N_SCANS):
        t = SCANS[i][6]
        if i and t is not None:
            out += dht(TABLE_IDS[t], tables[t])
        out += sos(i) + segs[i]
    return out + b'\xff\xd9'


def prefix_of(baseline_header):
    """The bytes of a baseline header up to its first DHT segment, its SOF0 marker made SOF2."""
    at = baseline_header.index(b'\xff\xc4')
    head = baseline_header[:at]
    sof = head.rindex(b'\xff\xc0')
    return head[:sof] + b'\xff\xc2' + head[sof + 2:]


def encode(coefs, h, w, hs, vs, prefix, restart_interval=0, stats=None):
    """-> (whole file, tables (10, 272), histograms (10, 257), [10 segments])."""
    items = all_items(coefs, h, w, hs, vs, restart_interval, stats)
    hist = histograms(items)
    tables, status = opt.optimal_tables(hist)
    assert not status.any()
    segs, st = segments(items, tables, stats)
    assert st == 0
    return assemble(prefix, segs, tables, restart_interval), tables, hist, segs

