"""The cases of the l3ic route tests (test_l3ic_cases.py on the CPU, test_gpu_l3ic_routes.py on the GPU) and their reference halves.
Every case carries an id that names the route its data takes through csrc/l3ic.hip; the routes are computed here from the plain
reference tests/l3ic_ref.py alone (normalisation branch, lane count, payload kind, which of the two RAW exits), so the self-test
can hold each id to its data.  Cases are built by construction or by a seeded search on the CPU; nothing here needs a GPU.

Operand rules.  Encoder layers are uint8 index layers with a prescribed histogram, shuffled with a fixed seed (the order decides
the words, not the route).  Decoder payloads are bytes: reference encodings with the encoder's and with foreign lane counts, forged
but valid tables, and damaged payloads whose status word is l3ic_ref.decode_status.  Quantiser operands are float32 values planted
on code-book entries, on the float32 midpoints between them, beyond both ends, -0.0 and +-3e38 (every squared distance inf), over
sorted, unsorted and repeated code-books; the reference is the kernel's arithmetic in numpy float32, first minimum."""
import functools
import struct
from collections import namedtuple

import numpy as np

import l3ic_ref as ref

M = ref.M
LANE_SIZES = (4095, 4096, 8191, 8192, 16383, 16384, 32767, 32768, 65535)


# ---- routes, computed from the reference -------------------------------------------------------------------------------------
def raw_frequencies(counts):
    n = int(sum(int(v) for v in counts))
    return [max(1, int(v) * M // n) if v > 0 else 0 for v in counts]


def surplus_parts(f, r):
    """The closed form the encoder's comment states: the lowest level v with D(v) = sum(max(0, f - v)) <= r, and left = r - D(v)."""
    lo, hi = 1, M
    while lo < hi:
        mid = (lo + hi) >> 1
        if sum(max(0, x - mid) for x in f) <= r:
            hi = mid
        else:
            lo = mid + 1
    return lo, r - sum(max(0, x - lo) for x in f)


def closed_form_normalise(counts):
    """l3ic_encode_kernel's normalisation restated from its comments: the whole deficit to the largest count (lowest index on
    ties); a surplus in closed form - every f above v comes down to v, then the first `left` symbols at v, in index order, go to
    v - 1."""
    c = [int(v) for v in counts]
    f = raw_frequencies(c)
    total = sum(f)
    if total < M:
        key = max((c[s] << 8) | (255 - s) for s in range(len(c)) if c[s])
        f[255 - (key & 255)] += M - total
    elif total > M:
        v, left = surplus_parts(f, total - M)
        before = 0
        for s in range(len(f)):
            if f[s] >= v:
                f[s] = v - 1 if before < left else v
                before += 1
    return f


def norm_route(counts):
    """'exact' | 'deficitD[-tie2]' | 'surplusR-leftX[-tie3][-levelsY]' of a histogram (symbol s sits in the encoder's lane s // 4)."""
    c = [int(v) for v in counts]
    f = raw_frequencies(c)
    total = sum(f)
    if total == M:
        return 'exact'
    if total < M:
        top = [s for s, v in enumerate(c) if v == max(c)]
        return 'deficit{}'.format(M - total) + ('-tie2' if len({s // 4 for s in top}) >= 2 else '')
    v, left = surplus_parts(f, total - M)
    at = {s // 4 for s, x in enumerate(f) if x >= v}
    levels = len({x for x in f if x > v}) + (1 if left else 0)
    return 'surplus{}-left{}'.format(total - M, left) + ('-tie3' if left and len(at) >= 3 else '') + \
        ('-levels{}'.format(levels) if levels >= 2 else '')


def layer_route(sym, k=256):
    """'rle' | 'rans' | 'raw-upfront' (the header alone reaches n: max_words < 0) | 'raw-midloop' (the words reach it) and the
    distance of the rANS payload from n (None for RLE)."""
    sym = np.asarray(sym, np.uint8).ravel()
    n = sym.size
    if np.all(sym == sym[0]):
        return 'rle', None
    f = ref.normalise(np.bincount(sym, minlength=256))
    if 3 + ref.table_bytes(f) + 4 * ref.lanes_for(n) >= n:
        return 'raw-upfront', None
    size = len(reference_rans(sym.tobytes()))
    return ('rans' if size < n else 'raw-midloop'), size - n


@functools.lru_cache(maxsize=None)
def reference_rans(sym_bytes, lanes=None):
    return ref.rans_encode(np.frombuffer(sym_bytes, np.uint8), 256, lanes=lanes)


@functools.lru_cache(maxsize=None)
def reference_payload(sym_bytes):
    """ref.encode_layer, once per layer and process (the pure-Python coder takes ~0.2 s at 65535 symbols)."""
    sym = np.frombuffer(sym_bytes, np.uint8)
    kind, _ = layer_route(sym)
    if kind == 'rle':
        return struct.pack('<HB', sym.size, int(sym[0]))
    return reference_rans(sym_bytes) if kind == 'rans' else sym_bytes


def route_id(sym):
    """The full route of an encoder layer: lanes / normalisation branch / payload kind[distance from n]."""
    sym = np.asarray(sym, np.uint8)
    kind, d = layer_route(sym)
    if kind == 'rle':
        return 'L{}/rle'.format(ref.lanes_for(sym.size))
    tail = kind if d is None or abs(d) > 1 else '{}{:+d}'.format(kind, d)
    return 'L{}/{}/{}'.format(ref.lanes_for(sym.size), norm_route(np.bincount(sym, minlength=256)), tail)


# ---- encoder cases ----------------------------------------------------------------------------------------------------------------
Enc = namedtuple('Enc', 'id n sym')            # id = '<what>:<route_id>'


def layer_of(counts, seed):
    """A layer with exactly this histogram, shuffled."""
    counts = np.asarray(counts, np.int64)
    return np.random.default_rng(seed).permutation(np.repeat(np.arange(counts.size), counts).astype(np.uint8))


def _hist(pairs):
    c = [0] * 256
    for s, v in pairs.items():
        c[s] = v
    return c


def _laplace(rng, n, k, scale):
    p = np.exp(-np.abs(np.arange(k) - (k - 1) / 2) / scale)
    return rng.choice(k, n, p=p / p.sum()).astype(np.uint8)


def adversarial_counts():
    return [1] * 200 + [584] * 39 + [576] * 17


@functools.lru_cache(maxsize=None)
def surplus_search():
    """The smallest n > 4096 at which a family of histograms takes each surplus route: {'surplus1' | 'left0' | 'tie3' |
    'levels2': counts}.  The family: m singletons (f = 1 each, which is what makes a surplus) and j large symbols 31 apart - so
    in j different lanes - that share the other n - m symbols evenly (the first (n - m) % j one more), j = 1 .. 8, m = 256 - j
    down to 160; with `skew` the first large symbol takes a quarter of the second's count on top (two levels)."""
    want = {'surplus1': lambda r: r.startswith('surplus1-'),
            'left0': lambda r: '-left0' in r and not r.startswith('surplus1-'),
            'tie3': lambda r: '-tie3' in r,
            'levels2': lambda r: '-levels' in r and '-left0' in r}
    found = {}
    for n in range(4097, 6000):
        for j in range(1, 9):
            big = [7 + 31 * i for i in range(j)]
            for m in (256 - j, 240, 200, 160):
                small = [s for s in range(256) if s not in big][:min(m, 256 - j)]
                for skew in (False, True):
                    share = [(n - len(small)) // j + (1 if i < (n - len(small)) % j else 0) for i in range(j)]
                    if skew and j >= 2:
                        share[0], share[1] = share[0] + share[1] // 4, share[1] - share[1] // 4
                    c = _hist(dict([(s, v) for s, v in zip(big, share)] + [(s, 1) for s in small]))
                    if sum(raw_frequencies(c)) <= M:
                        continue
                    r = norm_route(c)
                    for key, test in want.items():
                        if key not in found and test(r):
                            found[key] = c
        if len(found) == len(want):
            break
    return found


@functools.lru_cache(maxsize=None)
def choice_search():
    """Seeded default_rng layers whose rANS payload is exactly n - 1, n and n + 1 bytes: {-1 | 0 | 1: layer}, the first hit of
    each over n = 12 .. 63, k = 2 .. 8, 40 seeds."""
    found = {}
    for n in range(12, 64):
        for k in range(2, 9):
            for seed in range(40):
                sym = np.random.default_rng(1000 * n + 10 * k + seed).integers(0, k, n).astype(np.uint8)
                kind, d = layer_route(sym)
                if d in (-1, 0, 1) and d not in found:
                    found[d] = sym
            if len(found) == 3:
                return found
    return found


@functools.lru_cache(maxsize=None)
def encoder_cases():
    out = []

    def add(what, sym):
        sym = np.ascontiguousarray(sym, np.uint8)
        out.append(Enc('{}:{}'.format(what, route_id(sym)), sym.size, sym))

    # normalisation: deficit, exact
    add('tie-5-200', layer_of(_hist({5: 3, 200: 3, 100: 1}), 1))                       # deficit 1, the maximum in lanes 1 and 50
    add('tie-5-200-many', layer_of(_hist(dict([(5, 40), (200, 40)] + [(s, 1) for s in range(60, 83)])), 2))
    add('tie-200-first', layer_of(_hist({3: 2, 200: 5, 201: 5, 250: 5}), 3))           # a tie inside one lane and across two
    add('deficit1', layer_of(_hist({0: 1, 1: 2}), 4).repeat(4))                       # 1365 + 2730 = 4095
    add('exact', layer_of(_hist({9: 12, 10: 4}), 5))
    # normalisation: surplus
    for key, counts in sorted(surplus_search().items()):
        add(key, layer_of(counts, 6))
    # table bytes (n = 4096: the counts are the frequencies)
    add('varint-127-128', layer_of(_hist({30: 127, 31: 128, 32: 3841}), 7))
    add('zeros-inside', layer_of(_hist({10: 1000, 13: 96, 40: 3000}), 8))
    add('a0-b255', layer_of(_hist({0: 4000, 255: 96}), 9))
    add('b-a+1', layer_of(_hist({77: 100, 78: 3996}), 10))
    add('row-boundary', layer_of(_hist({0: 64, 1: 1984, 2: 2048}), 11))                # symbols starting on slots 64 and 2048
    add('f-1-4095', layer_of(_hist({3: 1, 4: 4095}), 12))
    add('f-4095-1', layer_of(_hist({3: 4095, 4: 1}), 13))
    # layer choice
    for d, sym in sorted(choice_search().items()):
        add('choice{:+d}'.format(d), sym)
    for n in (4, 11):
        add('two-symbols', np.array([0] + [1] * (n - 1), np.uint8))                   # header >= n: RAW before the loop
    add('two-symbols', np.array([0] + [1] * 11, np.uint8))                            # n = 12: max_words = 0 and no word needed
    add('uniform256', np.random.default_rng(14).permutation(np.arange(300) % 256).astype(np.uint8))
    add('rle', np.full(4, 255, np.uint8))
    add('rle', np.full(65535, 0, np.uint8))
    # lanes: at every size one skewed layer (n % L != 0 wherever L > 1 allows it: the odd sizes) and one of 256 symbols
    for n in LANE_SIZES:
        rng = np.random.default_rng(n)
        add('laplace32', _laplace(rng, n, 32, 1.5))
        add('laplace256', _laplace(rng, n, 256, 30.0))
    add('adversarial', layer_of(adversarial_counts(), 15))
    add('singletons255', layer_of(_hist(dict([(0, 65535 - 255)] + [(s, 1) for s in range(1, 256)])), 16))
    add('uniform256', np.random.default_rng(17).integers(0, 256, 65535).astype(np.uint8))
    return out


def encoder_groups():
    """{n: [Enc]}: the cases of one size go into one encode call as separate streams."""
    groups = {}
    for c in encoder_cases():
        groups.setdefault(c.n, []).append(c)
    return groups


ENCODER_ROUTES = [       # (name, test on a case id) - every one must be reached (test_l3ic_cases.py counts them)
    ('deficit, maximum tied in two lanes', lambda i: '-tie2/' in i),
    ('deficit of 1', lambda i: '/deficit1/' in i or '/deficit1-' in i),
    ('exact sum', lambda i: '/exact/' in i),
    ('surplus of 1', lambda i: '/surplus1-' in i),
    ('surplus, left == 0', lambda i: '/surplus' in i and '-left0' in i),
    ('surplus, left > 0 over three lanes', lambda i: '-tie3' in i),
    ('surplus, two levels', lambda i: '-levels' in i),
    ('rANS at n - 1', lambda i: i.endswith('/rans-1')),
    ('RAW at n', lambda i: i.endswith('/raw-midloop+0')),
    ('RAW at n + 1', lambda i: i.endswith('/raw-midloop+1')),
    ('RAW before the loop', lambda i: i.endswith('/raw-upfront')),
    ('RAW inside the loop', lambda i: '/raw-midloop' in i),
    ('RLE', lambda i: i.endswith('/rle')),
] + [('L = {}'.format(l), lambda i, l=l: ':L{}/'.format(l) in i and '/rans' in i) for l in (1, 2, 4, 8, 16)]


# ---- many streams -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stream_pool():
    """16-symbol layers by payload length: {3 (RLE), 11 .. 15 (rANS), 16 (RAW): [layers]}, from a seeded search."""
    pool = {3: [np.full(16, s, np.uint8) for s in (0, 9, 255)]}
    rng = np.random.default_rng(16)
    for _ in range(600):
        k = int(rng.integers(2, 5))
        p = rng.dirichlet(np.full(k, 0.6))
        sym = rng.choice(rng.permutation(256)[:k], 16, p=p).astype(np.uint8)
        size = len(reference_payload(sym.tobytes()))
        if size != 3 and len(pool.setdefault(size, [])) < 6:
            pool[size].append(sym)
    return pool


@functools.lru_cache(maxsize=None)
def many_streams(count):
    """`count` streams of 16 symbols whose consecutive payload lengths differ: (idx (count, 16) uint8, [payload])."""
    pool = stream_pool()
    flat = [(size, sym) for size in sorted(pool) for sym in pool[size]]
    rng = np.random.default_rng(count)
    picks, last = [], -1
    for _ in range(count):
        j = int(rng.integers(0, len(flat)))
        while flat[j][0] == last:
            j = int(rng.integers(0, len(flat)))
        picks.append(j)
        last = flat[j][0]
    return np.stack([flat[j][1] for j in picks]), [reference_payload(flat[j][1].tobytes()) for j in picks]


MANY = (1024, 1025, 2500)


# ---- decoder: valid streams the encoder never writes ------------------------------------------------------------------------------
Dec = namedtuple('Dec', 'id n k payload sym')           # sym None: a damaged payload


def forged_single(lanes, a):
    """A valid rANS payload of one symbol with frequency 4096 (the encoder writes RLE instead): no words, every state 2^16."""
    return bytes([lanes, a, a, 0x80, 0x20]) + struct.pack('<I', ref.LOW) * lanes


@functools.lru_cache(maxsize=None)
def foreign_cases():
    out = []
    rng = np.random.default_rng(64)
    skew = rng.choice(4, 600, p=[0.85, 0.08, 0.05, 0.02]).astype(np.uint8)
    for lanes in (1, 3, 5, 63, 64):                      # n = 600: T = 600, 200, 120, 10 (ragged 33), 10 (ragged 24)
        out.append(Dec('L{}/n600'.format(lanes), 600, 4, ref.rans_encode(skew, 4, lanes=lanes), skew))
    out.append(Dec('L5/n40', 40, 4, ref.rans_encode(skew[:40], 4, lanes=5), skew[:40]))
    out.append(Dec('L3/n29', 29, 4, ref.rans_encode(skew[:29], 4, lanes=3), skew[:29]))       # ragged: 29 = 9 * 3 + 2
    # a rANS payload is shorter than n and holds 4 L bytes of states, so n > 4 L + 5: the shortest layer a lane count can decode
    for lanes in (1, 3, 5, 63, 64):
        n = 4 * lanes + 6
        out.append(Dec('L{}/forged-single/n{}'.format(lanes, n), n, 256, forged_single(lanes, 201), np.full(n, 201, np.uint8)))
        two = np.array(([0] * 7 + [1]) * n, np.uint8)[:n + 4]
        out.append(Dec('L{}/shortest-two/n{}'.format(lanes, n + 4), n + 4, 2, ref.rans_encode(two, 2, lanes=lanes), two))
    tables = {'row-boundary': {0: 64, 1: 1984, 2: 2048}, 'f-1-4095': {3: 1, 4: 4095}, 'f-4095-1': {3: 4095, 4: 1},
              'row-boundary-many': dict((s, 64) for s in range(64))}
    for name, pairs in sorted(tables.items()):
        sym = layer_of(_hist(pairs), 65)
        for lanes in (2, 3, 64):                         # 2 is the encoder's own count at 4096
            out.append(Dec('L{}/{}'.format(lanes, name), 4096, 64, ref.rans_encode(sym, 64, lanes=lanes), sym))
    return out


# ---- decoder: damaged payloads --------------------------------------------------------------------------------------------------------
def _table(fs):
    return b''.join(ref._varint(v) for v in fs)


def _states(lanes, x=ref.LOW):
    return struct.pack('<I', x) * lanes


@functools.lru_cache(maxsize=None)
def damaged_bases():
    """Three valid payloads: (n, k, payload, sym) - one lane with few symbols, two lanes at 4096, a foreign 64 lanes."""
    rng = np.random.default_rng(600)
    a = rng.choice(4, 600, p=[0.7, 0.15, 0.1, 0.05]).astype(np.uint8)
    b = _laplace(rng, 4096, 32, 1.5)
    c = rng.choice(8, 2000, p=np.arange(8, 0, -1) / 36).astype(np.uint8)
    return [(600, 4, ref.rans_encode(a, 4), a), (4096, 32, ref.rans_encode(b, 32), b), (2000, 8, ref.rans_encode(c, 8, lanes=64), c)]


def table_end(p):
    """Offset of the states of a well-formed rANS payload."""
    pos = 3
    for _ in range(p[1], p[2] + 1):
        pos += 2 if p[pos] & 0x80 else 1
    return pos


@functools.lru_cache(maxsize=None)
def damaged_built():
    """Payloads built for one status bit each and for several at once, all for the first base's layer size and code-book
    (n = 600, k = 4): [Dec].  The id is '<status>/<what>' with the status as bit names joined by '+' in bit order, 'valid', or
    'any' where only l3ic_ref.decode_status says; the self-test holds the ids to decode_status."""
    n, k, good, _ = damaged_bases()[0]
    raw = bytes([0, 1, 2, 3] * 150)
    built = [
        ('READ/longer-than-n', bytes(n + 1)),
        ('READ/len65535', bytes(65535)),
        ('LANES/0', bytes([0]) + good[1:]),
        ('LANES/65', bytes([65]) + good[1:]),
        ('RANGE/a>b', bytes([1, 2, 1]) + good[3:]),
        ('RANGE/zero-first', bytes([1, 0, 2]) + _table([0, 4000, 96]) + _states(1)),
        ('RANGE/zero-last', bytes([1, 0, 2]) + _table([4000, 96, 0]) + _states(1)),
        ('SYMBOL/raw', raw[:17] + bytes([4]) + raw[18:]),
        ('SYMBOL/rle', struct.pack('<HB', n, 4)),
        ('SYMBOL/b>=k', bytes([1, 0, 4]) + _table([4092, 1, 1, 1, 1]) + _states(1)),
        ('FREQ/4095', bytes([1, 0, 1]) + _table([4000, 95]) + _states(1)),
        ('VARINT/sum-4096', bytes([1, 0, 1, 0xa0, 0x9f, 96]) + _states(1)),          # 0x20 | 0x1f << 7 = 4000 under a third-byte flag
        ('ODD/one-more-byte', good + b'\0'),
        ('UNUSED/one-more-word', good + b'\0\0'),
        ('STATE/forged-single', bytes([2, 1, 1, 0x80, 0x20]) + _states(1) + _states(1, ref.LOW + 1)),
        ('RLE/count', struct.pack('<HB', n - 1, 3)),
        ('valid/raw', raw),
        ('valid/rle', struct.pack('<HB', n, 3)),
        ('valid/forged-single', forged_single(64, 3)),
        # several bits at once
        ('READ+LANES/len0', b''),
        ('READ/len1', bytes([1])),
        ('READ+LANES/len1', bytes([200])),
        ('READ+RANGE/len2', bytes([1, 3])),
        ('READ/len2', bytes([1, 0])),
        ('LANES+RANGE+SYMBOL/header', bytes([0, 9, 8]) + good[3:]),
        ('SYMBOL+RLE/both', struct.pack('<HB', 0, 255)),
        ('ODD+UNUSED/three-more-bytes', good + b'\0\0\0'),
        ('RANGE+FREQ/all-zero', bytes([1, 0, 1]) + _table([0, 0]) + _states(1)),
        ('RANGE+FREQ/overflow-at-b', bytes([1, 0, 1]) + _table([4000, 97]) + _states(1)),   # the table ends where the sum passes 4096
        ('RANGE+FREQ+VARINT/16383', bytes([1, 0, 1, 0xff, 0xff, 96]) + _states(1)),
        ('any/table-cut', good[:4]),
        ('any/states-cut', good[:table_end(good) + 2]),
        ('any/words-cut', good[:-2]),
        ('any/words-cut-odd', good[:-1]),
        ('any/64-lanes-8-states', bytes([64, 0, 1]) + _table([4000, 96]) + _states(8)),
    ]
    return [Dec(name, n, k, p, None) for name, p in built]


@functools.lru_cache(maxsize=None)
def damaged_small():
    """n_sym below the lane count (n = 40, L = 64: lanes 40 .. 63 hold states and take no symbol), reachable only through
    damage, as 4 L state bytes do not fit a payload shorter than n."""
    head = bytes([64, 0, 1]) + _table([4000, 96])
    return [Dec('n<L/' + name, 40, 2, p, None) for name, p in [
        ('states-cut', head + _states(8)), ('states-cut-odd', head + _states(8) + b'\1'), ('no-states', head),
        ('valid-forged-L8', forged_single(8, 1))]]


@functools.lru_cache(maxsize=None)
def damaged_family():
    """70 seeded single-bit flips and 10 truncations of each base payload: [(base index, Dec)], 240 in all."""
    rng = np.random.default_rng(20241018)
    out = []
    for bi, (n, k, good, _) in enumerate(damaged_bases()):
        for j in range(70):
            bit = int(rng.integers(0, 8 * len(good))) if j >= 30 else int(rng.integers(0, 8 * min(len(good), 16 + 4 * good[0])))
            p = bytearray(good)
            p[bit >> 3] ^= 1 << (bit & 7)
            out.append((bi, Dec('base{}|flip{}'.format(bi, bit), n, k, bytes(p), None)))
        for cut in sorted({int(v) for v in rng.integers(0, len(good), 7)} | {4, len(good) - 1, len(good) - 2}):
            out.append((bi, Dec('base{}|cut{}'.format(bi, cut), n, k, good[:cut], None)))
    return out


# ---- quantiser ------------------------------------------------------------------------------------------------------------------------
Quant = namedtuple('Quant', 'id z cb bad')           # z (images, 1, n_sym, c) float32, cb (k,) float32, bad: a non-finite value planted

CODEBOOKS = {
    'sorted32': np.arange(-15, 17, dtype=np.float32),
    'unsorted9': np.array([1.0, -7.0, 12.0, -0.25, 3.5, 0.0, -2.5, 0.1, -2.0], np.float32),
    'repeated6': np.array([2.0, -1.0, 2.0, 0.5, -1.0, 0.5], np.float32),
    'k1': np.array([0.75], np.float32),
    'k2': np.array([-0.5, 0.5], np.float32),
    'k256': (np.arange(256, dtype=np.float32) - 127) / 8,
}


def quantise_reference(z, cb):
    """float32(cb - v), squared in float32, the first minimum (strict <): (images, c, n_sym) uint8 - the kernel's arithmetic."""
    z, cb = np.asarray(z, np.float32), np.asarray(cb, np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        d = (cb[None, :] - z.reshape(-1, 1)).astype(np.float32)
        d2 = (d * d).astype(np.float32)
    idx = np.where(np.isnan(d2).any(axis=1), 0, np.argmin(np.where(np.isnan(d2), np.inf, d2), axis=1)).astype(np.uint8)
    b, _, n_sym, c = z.shape
    return idx.reshape(b, n_sym, c).transpose(0, 2, 1).copy()


def quantise_operand(cb, images, n_sym, c, seed):
    cb = np.asarray(cb, np.float32)
    rng = np.random.default_rng(seed)
    span = float(cb.max() - cb.min()) + 2.0
    z = (rng.standard_normal(images * n_sym * c) * span / 3 + float(cb.mean())).astype(np.float32)
    u = np.unique(cb)
    plant = list(cb) + list(((u[1:] + u[:-1]) / np.float32(2)).astype(np.float32)) + \
        [cb.min() - 0.75, cb.max() + 0.75, -1e3, 1e3, -0.0, 0.0, 3e38, -3e38, np.nextafter(np.float32(cb[0]), np.float32(99))]
    at = rng.permutation(z.size)[:len(plant)] if z.size >= len(plant) else np.arange(z.size)
    z[at] = np.array(plant, np.float32)[:len(at)]
    return z.reshape(images, 1, n_sym, c)


@functools.lru_cache(maxsize=None)
def quantiser_cases():
    out = []

    def add(name, cbname, images, n_sym, c, seed, bad_at=None):
        z = quantise_operand(CODEBOOKS[cbname], images, n_sym, c, seed)
        if bad_at is not None:
            z[bad_at[0], 0, bad_at[1], bad_at[2]] = bad_at[3]
        out.append(Quant('{}/{}/b{}-n{}-c{}'.format(name, cbname, images, n_sym, c), z, CODEBOOKS[cbname], bad_at is not None))

    for n_sym in (1, 63, 64, 65, 200):
        add('pixels', 'sorted32', 3, n_sym, 3, n_sym)
    for c in (1, 3, 255, 256):
        add('features', 'unsorted9', 3, 65, c, 100 + c)
    for cbname in ('k1', 'k2', 'k256', 'repeated6', 'unsorted9'):
        add('codebook', cbname, 3, 130, 5, 200)
    add('nonfinite-first', 'sorted32', 3, 65, 3, 300, (0, 0, 0, np.nan))
    add('nonfinite-last', 'sorted32', 3, 65, 3, 301, (2, 64, 2, np.inf))
    add('nonfinite-tail', 'sorted32', 3, 65, 3, 302, (1, 64, 1, -np.inf))
    add('lds128k', 'sorted32', 3, 65, 2048, 400)               # 64 c = 128 KiB of dynamic LDS
    return out
