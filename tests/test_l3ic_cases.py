"""Self-test of tests/l3ic_cases.py (no GPU): every case takes the route its id names - recomputed here from l3ic_ref's coder, not
from the helpers that built the id - every route of csrc/l3ic.hip the list is meant to reach is reached (a counter, printed with
pytest -s), l3ic_ref.decode_status agrees with l3ic_ref.decode_layer, every status bit occurs alone, the closed-form surplus rule the
kernel's comment states equals the reference's loop, the numpy float32 quantiser equals scipy's vq, and the comparisons of
test_gpu_l3ic_routes.py reject stand-ins with the bugs they are there to catch."""
import collections

import numpy as np
import pytest
from scipy.cluster.vq import vq

import l3ic_cases as cases
import l3ic_ref as ref

# the case list, pinned: a change of a builder or a seed that moves a case to another route shows up here
ENCODER_IDS = [
    'tie-5-200:L1/deficit1-tie2/raw-upfront', 'tie-5-200-many:L1/deficit19-tie2/raw-upfront',
    'tie-200-first:L1/deficit3-tie2/raw-upfront', 'deficit1:L1/deficit1/rans-1', 'exact:L1/exact/rans',
    'left0:L2/surplus2-left0/rans', 'levels2:L2/surplus3-left0-levels2/rans', 'surplus1:L2/surplus1-left0/rans',
    'tie3:L2/surplus1-left1-tie3/rans',
    'varint-127-128:L2/exact/rans', 'zeros-inside:L2/exact/rans', 'a0-b255:L2/exact/rans', 'b-a+1:L2/exact/rans',
    'row-boundary:L2/exact/rans', 'f-1-4095:L2/exact/rans', 'f-4095-1:L2/exact/rans',
    'choice-1:L1/exact/rans-1', 'choice+0:L1/deficit1/raw-midloop+0', 'choice+1:L1/deficit2/raw-midloop+1',
    'two-symbols:L1/exact/raw-upfront', 'two-symbols:L1/deficit1/raw-upfront', 'two-symbols:L1/deficit1/rans-1',
    'uniform256:L1/deficit152-tie2/raw-midloop', 'rle:L1/rle', 'rle:L16/rle',
    'laplace32:L1/deficit1/rans', 'laplace256:L1/deficit1/rans', 'laplace32:L2/exact/rans', 'laplace256:L2/exact/rans',
    'laplace32:L2/deficit4/rans', 'laplace256:L2/deficit56/rans', 'laplace32:L4/deficit1/rans', 'laplace256:L4/deficit62/rans',
    'laplace32:L4/deficit6/rans', 'laplace256:L4/deficit87/rans', 'laplace32:L8/deficit6/rans', 'laplace256:L8/deficit87/rans',
    'laplace32:L8/deficit5/rans', 'laplace256:L8/deficit99/rans', 'laplace32:L16/deficit3/rans', 'laplace256:L16/deficit107/rans',
    'laplace32:L16/deficit3/rans', 'laplace256:L16/deficit112/rans',
    'adversarial:L16/surplus175-left24-tie3-levels3/rans', 'singletons255:L16/surplus239-left0/rans',
    'uniform256:L16/deficit122/raw-midloop']
SURPLUS_SIZES = {'surplus1': 4113, 'tie3': 4115, 'left0': 4129, 'levels2': 4147}          # the smallest n of the searched family


def _names(status):
    return '+'.join(name for bit, name in sorted(ref.E_NAMES.items()) if status & bit) or 'valid'


# ---- the ids against the data ----------------------------------------------------------------------------------------------------
def test_encoder_case_list_is_the_pinned_one():
    assert [c.id for c in cases.encoder_cases()] == ENCODER_IDS
    assert {c.id.split(':')[0]: c.n for c in cases.encoder_cases() if c.id.split(':')[0] in SURPLUS_SIZES} == SURPLUS_SIZES
    assert sorted(cases.encoder_groups()) == sorted({4, 7, 11, 12, 14, 15, 16, 17, 103, 300, 4096, 4113, 4115, 4129, 4147} |
                                                    set(cases.LANE_SIZES))


@pytest.mark.parametrize('case', cases.encoder_cases(), ids=[c.id for c in cases.encoder_cases()])
def test_encoder_id_names_the_route_of_its_data(case):
    """The route read off the reference coder itself: the payload ref.encode_layer writes, and ref.normalise's loop counted."""
    what, route = case.id.split(':')
    parts = route.split('/')
    sym, n = case.sym, case.n
    assert sym.dtype == np.uint8 and sym.size == n and 4 <= n <= 65535
    payload = ref.encode_layer(sym)
    assert payload == cases.reference_payload(sym.tobytes())
    assert np.array_equal(ref.decode_layer(payload, n), sym) and ref.decode_status(payload, n) == 0
    lanes = ref.lanes_for(n)
    assert parts[0] == 'L{}'.format(lanes)
    if lanes > 1 and n % 2:
        assert n % lanes != 0                                # the odd sizes end on a ragged step
    if parts[-1] == 'rle':
        assert len(payload) == 3 and len(set(sym.tolist())) == 1
        return
    counts = np.bincount(sym, minlength=256)
    raw = [max(1, int(v) * 4096 // n) if v else 0 for v in counts]
    f = ref.normalise(counts)
    moved = [s for s in range(256) if f[s] != raw[s]]
    if parts[1] == 'exact':
        assert sum(raw) == 4096 and not moved
    elif parts[1].startswith('deficit'):
        assert parts[1].split('-')[0] == 'deficit{}'.format(4096 - sum(raw)) and len(moved) == 1
        top = [s for s in range(256) if counts[s] == counts.max()]
        assert moved[0] == top[0]
        assert ('-tie2' in parts[1]) == (len({s // 4 for s in top}) >= 2)
    else:
        r = sum(raw) - 4096
        assert r > 0 and parts[1].startswith('surplus{}-'.format(r))
        cut = min(f[s] for s in moved)                        # the lowest value a lowered symbol ended on
        lowest = [s for s in moved if f[s] == cut]
        left = int(parts[1].split('-left')[1].split('-')[0])
        if left:                                              # `left` symbols went one below the level the others stopped at
            assert len(lowest) == left and all(f[s] >= cut for s in range(256) if raw[s] > cut)
            at = [s for s in range(256) if raw[s] > cut]
            assert lowest == at[:left]                        # ... the first ones in index order
            assert ('-tie3' in parts[1]) == (len({s // 4 for s in at}) >= 3)
        else:
            assert all(f[s] == cut for s in moved) and all(raw[s] <= cut for s in range(256) if s not in moved)
        if '-levels' in parts[1] and not left:
            assert len({raw[s] for s in moved}) >= 2
    hdr = 3 + ref.table_bytes(f) + 4 * lanes
    tail = parts[2]
    if tail.startswith('rans'):
        assert len(payload) < n and payload[0] == lanes and payload == ref.rans_encode(sym)
        assert tail == 'rans' + ('-1' if len(payload) == n - 1 else '')
    else:
        assert payload == sym.tobytes()
        if tail == 'raw-upfront':
            assert (n - hdr - 1) >> 1 < 0                     # max_words of the kernel
        else:
            d = len(ref.rans_encode(sym)) - n
            assert (n - hdr - 1) >> 1 >= 0 and d >= 0
            assert tail == 'raw-midloop' + ('{:+d}'.format(d) if d <= 1 else '')
    if what == 'varint-127-128':
        assert [v for v in f if v] == [127, 128, 3841] and payload[3:7] == bytes([127, 0x80, 0x01, 0x81])
    if what == 'zeros-inside':
        assert (payload[1], payload[2]) == (10, 40) and f[11] == f[12] == 0 and payload[5:7] == b'\0\0'
    if what == 'a0-b255':
        assert (payload[1], payload[2]) == (0, 255) and ref.table_bytes(f) == 257
    if what == 'b-a+1':
        assert payload[2] == payload[1] + 1


def test_every_route_is_reached():
    reached = collections.OrderedDict()
    ids = [c.id for c in cases.encoder_cases()]
    for name, test in cases.ENCODER_ROUTES:
        reached['encode: ' + name] = sum(1 for i in ids if test(i))
    reached['encode: 127 | 128 varint switch'] = sum(1 for i in ids if i.startswith('varint-127-128'))
    reached['encode: zero frequencies inside a..b'] = sum(1 for i in ids if i.startswith(('zeros-inside', 'a0-b255')))
    reached['encode: b = a + 1'] = sum(1 for i in ids if i.startswith(('b-a+1', 'f-1-4095', 'f-4095-1')))
    for n in cases.LANE_SIZES:
        reached['encode: n = {}'.format(n)] = sum(1 for c in cases.encoder_cases() if c.n == n and '/rans' in c.id)
    for n in cases.LANE_SIZES[2::2] + (65535,):
        reached['encode: ragged last step at n = {}'.format(n)] = int(n % ref.lanes_for(n) != 0 and ref.lanes_for(n) > 1)
    reached['encode: several histograms in one call'] = sum(1 for g in cases.encoder_groups().values() if len(g) >= 3)
    for count in cases.MANY:
        idx, payloads = cases.many_streams(count)
        sizes = [len(p) for p in payloads]
        assert idx.shape == (count, 16) and all(a != b for a, b in zip(sizes, sizes[1:]))
        assert {3, 16} <= set(sizes) and len(set(sizes) & {11, 12, 13, 14, 15}) >= 3 and set(sizes) <= {3, 11, 12, 13, 14, 15, 16}
        reached['scan: {} streams, per = {}, idle threads {}'.format(count, -(-count // 1024), 1024 - -(-count // -(-count // 1024)))] = 1
    foreign = cases.foreign_cases()
    for lanes in (1, 3, 5, 63, 64):
        reached['decode: foreign L = {}'.format(lanes)] = sum(1 for d in foreign if d.payload[0] == lanes)
    reached['decode: ragged last step, L = 64'] = sum(1 for d in foreign if d.payload[0] == 64 and d.n % 64)
    reached['decode: shortest layer of a lane count (n = 4 L + 6)'] = sum(1 for d in foreign if d.n == 4 * d.payload[0] + 6)
    reached['decode: forged single-symbol table, f = 4096'] = sum(1 for d in foreign if 'forged-single' in d.id)
    reached['decode: symbol starting on a row boundary'] = sum(1 for d in foreign if 'row-boundary' in d.id)
    reached['decode: f = {1, 4095}'] = sum(1 for d in foreign if 'f-1-4095' in d.id)
    reached['decode: f = {4095, 1}'] = sum(1 for d in foreign if 'f-4095-1' in d.id)
    damaged = cases.damaged_built() + cases.damaged_small() + [d for _, d in cases.damaged_family()]
    status = [ref.decode_status(d.payload, d.n, d.k) for d in damaged]
    for bit, name in sorted(ref.E_NAMES.items()):
        reached['decode: {} alone'.format(name)] = sum(1 for s in status if s == bit)
    reached['decode: several bits'] = sum(1 for d, s in zip(cases.damaged_built(), [ref.decode_status(d.payload, d.n, d.k) for d in cases.damaged_built()])
                                          if bin(s).count('1') >= 2)
    reached['decode: flips and truncations'] = len(cases.damaged_family())
    for size in (0, 1, 2):
        reached['decode: payload of {} bytes'.format(size)] = sum(1 for d in damaged if len(d.payload) == size)
    reached['decode: n_sym < L (damaged only)'] = sum(1 for d in cases.damaged_small() if d.n < d.payload[0] and
                                                      ref.decode_status(d.payload, d.n, d.k))
    quant = cases.quantiser_cases()
    for n_sym in (1, 63, 64, 65, 200):
        reached['quantise: n_sym = {}, 3 images'.format(n_sym)] = sum(1 for q in quant if q.z.shape[:3] == (3, 1, n_sym))
    for c in (1, 3, 255, 256, 2048):
        reached['quantise: c = {}'.format(c)] = sum(1 for q in quant if q.z.shape[3] == c)
    for k in (1, 2, 256):
        reached['quantise: k = {}'.format(k)] = sum(1 for q in quant if q.cb.size == k)
    reached['quantise: unsorted code-book'] = sum(1 for q in quant if np.any(np.diff(q.cb) < 0))
    reached['quantise: repeated entries'] = sum(1 for q in quant if np.unique(q.cb).size < q.cb.size)
    reached['quantise: non-finite value'] = sum(1 for q in quant if q.bad)
    print('\n'.join(['', 'l3ic routes reached (cases per route)'] + ['  {:62s} {}'.format(k, v) for k, v in reached.items()]))
    assert all(v >= 1 for v in reached.values()), [k for k, v in reached.items() if v < 1]
    assert reached['decode: several bits'] >= 3 and reached['decode: flips and truncations'] >= 200
    assert reached['quantise: non-finite value'] == 3


def test_a_rans_payload_needs_more_symbols_than_four_per_lane():
    """Why n_sym < L is no valid case: the states alone are 4 L bytes and a rANS payload is shorter than n_sym."""
    for lanes in range(1, 65):
        shortest = cases.forged_single(lanes, 0)
        assert len(shortest) == 4 * lanes + 5
        assert ref.decode_status(shortest, len(shortest) + 1) == 0
        assert ref.decode_status(shortest, len(shortest)) == 0                          # the same bytes as a RAW layer
        assert ref.decode_status(shortest, len(shortest) - 1) == ref.E_READ


# ---- decode_status -----------------------------------------------------------------------------------------------------------------
def _agree(d):
    status = ref.decode_status(d.payload, d.n, d.k)
    if status == 0:
        out = ref.decode_layer(d.payload, d.n, d.k)
        assert out.shape == (d.n,) and int(out.max()) < d.k, d.id
        if d.sym is not None:
            assert np.array_equal(out, d.sym), d.id
    else:
        with pytest.raises(ref.FormatError):
            ref.decode_layer(d.payload, d.n, d.k)
    return status


def test_decode_status_agrees_with_decode_layer():
    for d in cases.foreign_cases():
        assert _agree(d) == 0 and len(d.payload) < d.n, d.id
    seen = collections.Counter()
    for d in cases.damaged_built() + cases.damaged_small() + [d for _, d in cases.damaged_family()]:
        seen[_agree(d)] += 1
    assert len(seen) >= 15
    for n, k, payload, sym in cases.damaged_bases():
        assert ref.decode_status(payload, n, k) == 0 and np.array_equal(ref.decode_layer(payload, n, k), sym) and len(payload) < n


def test_built_payloads_have_the_status_they_are_named_for():
    alone = set()
    for d in cases.damaged_built():
        want, status = d.id.split('/')[0], ref.decode_status(d.payload, d.n, d.k)
        if want != 'any':
            assert _names(status) == want, d.id
        if bin(status).count('1') == 1:
            alone.add(status)
    assert alone == set(ref.E_NAMES)
    assert ref.E_NAMES == {1: 'READ', 2: 'LANES', 4: 'RANGE', 8: 'SYMBOL', 16: 'FREQ', 32: 'VARINT', 64: 'ODD', 128: 'UNUSED',
                           256: 'STATE', 512: 'RLE'}


def test_error_bits_are_the_headers():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'nimg.h')).read()
    found = {int(v): name for name, v in re.findall(r'#define NIMG_L3IC_E_(\w+) (\d+)', text)}
    assert found == ref.E_NAMES


# ---- the closed form of the surplus loop ------------------------------------------------------------------------------------------
def test_closed_form_normalisation_equals_the_loop():
    for c in cases.encoder_cases():
        counts = np.bincount(c.sym, minlength=256)
        assert cases.closed_form_normalise(counts) == ref.normalise(counts), c.id
    rng = np.random.default_rng(4096)
    branches = collections.Counter()
    for trial in range(3000):
        if trial % 3 == 0:                                   # any histogram
            k = int(rng.integers(2, 257))
            counts = rng.multinomial(int(rng.integers(4, 65536)), rng.dirichlet(np.full(k, rng.choice([0.05, 0.5, 5.0]))))
        else:                                                # singletons and a few large symbols: the family that has a surplus
            n, m, j = int(rng.integers(4097, 65536)), int(rng.integers(100, 251)), int(rng.integers(1, 6))
            pos = rng.permutation(256)
            share = rng.multinomial(n - m - j, rng.dirichlet(np.full(j, rng.choice([0.5, 5.0, 500.0])))) + 1
            counts = np.zeros(256, np.int64)
            counts[pos[:m]] = 1
            counts[pos[m:m + j]] = share
        total = sum(cases.raw_frequencies(counts))
        branches['deficit' if total < 4096 else 'surplus' if total > 4096 else 'exact'] += 1
        assert cases.closed_form_normalise(counts) == ref.normalise(counts), trial
    assert branches['surplus'] >= 1000 and branches['deficit'] >= 500, branches


# ---- the quantiser's reference ---------------------------------------------------------------------------------------------------
def test_quantise_reference_equals_scipy_vq():
    for q in cases.quantiser_cases():
        flat = q.z.reshape(-1)
        keep = np.abs(flat) < 1e18                           # vq refuses non-finite data; beyond 1e19 every float32 distance is inf
        got = cases.quantise_reference(q.z, q.cb)
        b, _, n_sym, c = q.z.shape
        assert got.shape == (b, c, n_sym) and got.dtype == np.uint8
        back = got.transpose(0, 2, 1).reshape(-1)
        assert np.array_equal(back[keep], vq(flat[keep], q.cb)[0]), q.id
        assert np.all(back[~keep] == 0), q.id                # every distance inf or NaN: no entry is ever strictly nearer
        assert q.bad == (not np.isfinite(flat).all())
        if q.z.size > 200:
            assert (~keep).sum() >= 2 and np.signbit(flat[flat == 0]).any()


# ---- the comparisons reject what they are there to catch -------------------------------------------------------------------------
def test_comparisons_reject_the_bugs_they_are_for():
    by_what = {c.id: c for c in cases.encoder_cases()}

    # deficit to the HIGHEST index among the largest counts
    def deficit_last(counts):
        c = [int(v) for v in counts]
        f = cases.raw_frequencies(c)
        if sum(f) < 4096:
            f[max(s for s in range(256) if c[s] == max(c))] += 4096 - sum(f)
        return f
    c = by_what['tie-5-200:L1/deficit1-tie2/raw-upfront']
    counts = np.bincount(c.sym, minlength=256)
    assert deficit_last(counts) != ref.normalise(counts) and deficit_last(counts)[200] == ref.normalise(counts)[5]

    # surplus: `left` symbols from the highest index down
    def surplus_last(counts):
        f = cases.raw_frequencies(counts)
        v, left = cases.surplus_parts(f, sum(f) - 4096)
        at = [s for s in range(256) if f[s] >= v]
        return [0 if not f[s] else f[s] if f[s] < v else v - 1 if s in at[len(at) - left:] else v for s in range(256)]
    c = by_what['tie3:L2/surplus1-left1-tie3/rans']
    counts = np.bincount(c.sym, minlength=256)
    assert sum(surplus_last(counts)) == 4096 and surplus_last(counts) != ref.normalise(counts)

    # rANS if not longer (<=) instead of strictly shorter
    c = by_what['choice+0:L1/deficit1/raw-midloop+0']
    assert len(ref.rans_encode(c.sym)) == c.n and ref.encode_layer(c.sym) != ref.rans_encode(c.sym)

    # a scan that sums one stream per thread: right up to 1024 streams, wrong from 1025
    def scan_one(lengths):
        per = -(-len(lengths) // 1024)
        out, run = [], 0
        for t in range(1024):
            mine = lengths[t * per:(t + 1) * per]
            o = run
            for v in mine:
                out.append(o)
                o += v
            run += mine[0] if len(mine) else 0
        return out
    for count in cases.MANY:
        lengths = [len(p) for p in cases.many_streams(count)[1]]
        true = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
        assert (scan_one(lengths) == true) == (count <= 1024)

    # a decoder that never reports one bit: every bit has a payload whose whole status it is
    for bit in ref.E_NAMES:
        assert any(ref.decode_status(d.payload, d.n, d.k) == bit for d in cases.damaged_built())

    # a quantiser that takes the LAST minimum, or measures |d| in float64
    q = next(q for q in cases.quantiser_cases() if q.id.startswith('codebook/repeated6'))
    d2 = (q.cb[None, :].astype(np.float64) - q.z.reshape(-1, 1)) ** 2
    last = (q.cb.size - 1 - np.argmin(d2[:, ::-1], axis=1)).astype(np.uint8)
    want = cases.quantise_reference(q.z, q.cb).transpose(0, 2, 1).reshape(-1)
    assert not np.array_equal(last, want)
