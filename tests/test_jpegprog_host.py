"""Progressive JPEG files on the host (no GPU): the plain Python restatement (tests/jpegprog_ref.py) against Pillow's progressive=True
and the committed golden files, what the case list reaches, the sequential core of csrc/jpegprog.h built into a stand-alone program
under AddressSanitizer and UBSan against the restatement and Pillow, and the host half of the product (the header pieces, the
keyword's defaults and refusals)."""
import importlib.util
import inspect
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_cases
import jpeg_ref as ref
import jpegopt_ref as oref
import jpegprog_cases as cases
import jpegprog_ref as pref
from neural_imaging_amd import ops
from neural_imaging_amd.compression import jpeg_helpers as jh


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------
def test_restatement_equals_golden():
    golden = cases.golden()
    assert list(golden) == cases.IDS
    for case in cases.QUICK:
        r = cases.reference(case)
        assert golden[case.name] == r.files, case.name
        for data, tables, segments in zip(r.files, r.tables, r.segments):       # and the file taken apart by its markers
            got_tables, got_segments = cases.split_file(data)
            assert np.array_equal(got_tables, tables) and got_segments == segments, case.name


def test_golden_layout():
    """SOF2 with the SOF0 body, the first DHT at offset 177 (246 with three quantisation tables), DRI in front of the first SOS, Cr in
    front of Cb."""
    for case in cases.QUICK:
        at = 246 if case.qtables == 'three' else 177
        for i, data in enumerate(cases.golden()[case.name]):
            assert data[at - 19:at - 15] == b'\xff\xc2\x00\x11' and data[at:at + 5] == b'\xff\xc4\x00' + data[at + 3:at + 4] + b'\x00', case.name
            sos = data.index(b'\xff\xda')
            assert (data[sos - 6:sos] == b'\xff\xdd\x00\x04' + case.ri.to_bytes(2, 'big')) == bool(case.ri), case.name
            order = [data[k + 5] for k in range(len(data) - 6) if data[k:k + 4] == b'\xff\xda\x00\x08']
            assert order[:4] == [1, 3, 2, 1], case.name
    assert sum(len(cases.golden()['g_' + case.name]) for case in jpeg_cases.GOLDEN_CASES) == 47


def test_golden_files_are_pillows():
    """Pillow writes the golden files, the same with optimize=True, and decodes each to the pixels of the baseline file."""
    pytest.importorskip('PIL.Image')
    spec = importlib.util.spec_from_file_location('make_jpegprog_golden', os.path.join(os.path.dirname(cases.GOLDEN), 'make_jpegprog_golden.py'))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    from PIL import Image
    golden = cases.golden()
    for case in cases.CASES:
        for i, img in enumerate(cases.build(case)):
            data, decoded = make.pillow(img, case)
            assert golden[case.name][i] == data, case.name
            if not case.slow:
                assert data == make.pillow(img, case, optimize=True)[0], case.name
            if case.kind == 'jpeg':
                baseline = jpeg_cases.golden()[case.arg][1][i]
                assert np.array_equal(decoded, np.asarray(Image.open(io.BytesIO(baseline)).convert('RGB'))), case.name
            elif not case.slow:
                assert np.array_equal(decoded, make.pillow(img, case, progressive=False)[1]), case.name
    assert os.path.getsize(cases.GOLDEN) <= max(os.path.getsize(os.path.join(os.path.dirname(cases.GOLDEN), f))
                                                for f in os.listdir(os.path.dirname(cases.GOLDEN)) if f != os.path.basename(cases.GOLDEN))


def test_case_list_reaches_every_path():
    """Every counter of the restatement is reached by a case that a Pillow file pins; the flat image (32768 luma blocks) is the one
    with a run of exactly 0x7fff blocks, then a run of 1."""
    total = dict.fromkeys(pref.COUNTERS, 0)
    for case in cases.CASES:
        r = cases.reference(case)
        assert r.files == cases.golden()[case.name], case.name
        for key, v in r.stats.items():
            total[key] += v
    assert all(total[key] > 0 for key in pref.COUNTERS), total
    flat = cases.reference(cases.by_name('flat_512x4096_q75_444'))
    assert flat.stats['flush_7fff'] == 8 and flat.stats['eobrun_cat0'] == 8
    for t in range(2, 10):
        assert flat.hists[0, t, 0xe0] == 1 and flat.hists[0, t, 0x00] == 1 and flat.hists[0, t].sum() == 2
    corr = cases.reference(cases.by_name('corr_32x160_q100_444'))
    assert corr.stats['flush_937'] >= 10 and cases.reference(cases.by_name('corr_32x160_q100_420')).stats['flush_937'] >= 10
    ragged = cases.reference(cases.by_name('mixed_37x53_q75_420_ri0'))
    assert ragged.coefs[0][0].shape[:2] == (5, 7) and ragged.stats['dummy_right'] and ragged.stats['dummy_bottom']
    for s in cases.synthetic()[:4]:
        stats = cases.synthetic_reference(s.name)[3]
        assert stats['zrl_first'] and stats['zrl_refine'] and stats['refine_tail_run'], s.name


# ---- 2. the sequential core under sanitizers, as a stand-alone program --------------------------------------------------------
@pytest.fixture(scope='module')
def host():
    try:
        cases.host_program(True)
    except subprocess.CalledProcessError as e:
        pytest.fail('the host program does not build with -fsanitize=address,undefined:\n' + e.stdout.decode())
    images, names = [], []
    for case in cases.CASES:
        hs, vs = ref.SUBSAMPLING[case.subsampling]
        for i, coef in enumerate(cases.flat(case)):
            images.append(cases.Image(case.h, case.w, hs, vs, case.ri, coef, None))
            names.append((case.name, i))
    for s in cases.synthetic():
        images.append(cases.Image(s.h, s.w, s.hs, s.vs, s.ri, s.flat, None))
        names.append((s.name, 0))
    damaged = _damaged()
    for _, im, _ in damaged:
        images.append(im)
    out, done = cases.host_results(images, sanitize=True)
    assert done.returncode == 0 and done.stderr == b'', done.stderr.decode()[-4000:]
    return dict(zip(names, out)), out[len(names):], damaged


def _damaged():
    """[(what, Image with given tables, the restatement's (segments, status))]: table sets the derive step must refuse or survive."""
    case = cases.by_name('mixed_37x53_q75_420_ri3')
    r = cases.reference(case)
    items = pref.all_items(r.coefs[0], case.h, case.w, 2, 2, case.ri)
    out = []
    for what, (t, k, v) in (('too many codes', (0, 0, 3)), ('too many codes in an AC table', (6, 1, 5)), ('more than 256 symbols', (9, 15, 255)),
                            ('the last code missing', (3, None, None)), ('no codes', (None, None, None))):
        tables = r.tables[0].copy()
        if t is None:
            tables[:] = 0
        elif k is None:
            tables[t, int(np.nonzero(tables[t, :16])[0][-1])] -= 1
        else:
            tables[t, k] = v
        out.append((what, cases.Image(case.h, case.w, 2, 2, case.ri, r.flat[0], tables), pref.segments(items, tables)))
    assert [o[2][1] for o in out] == [oref.ST_TABLE, oref.ST_TABLE, oref.ST_TABLE, oref.ST_SYMBOL, oref.ST_SYMBOL]
    return out


def test_host_program_equals_the_restatement_and_pillow(host):
    results, _, _ = host
    for case in cases.CASES:
        for i, data in enumerate(cases.golden()[case.name]):
            o = results[(case.name, i)]
            tables, segments = cases.split_file(data)
            assert o.status == 0 and np.array_equal(o.tables, tables) and o.segments == segments, case.name
            r = cases.reference(case)
            assert np.array_equal(o.hist, r.hists[i]) and np.array_equal(o.tables, r.tables[i]), case.name
    for s in cases.synthetic():
        hist, tables, segments, _ = cases.synthetic_reference(s.name)
        o = results[(s.name, 0)]
        assert o.status == 0 and np.array_equal(o.hist, hist) and np.array_equal(o.tables, tables) and o.segments == segments, s.name


def test_host_program_on_damaged_tables(host):
    _, got, damaged = host
    assert len(got) == len(damaged) == 5
    for o, (what, _, (segments, status)) in zip(got, damaged):
        assert o.status == status and o.segments == segments, what


# ---- 3. the host half of the product --------------------------------------------------------------------------------------------
def test_header_pieces():
    for name in ('g_smooth+noise+half_13x21_q95_420', 'mixed_37x53_q75_422_ri7', 'mixed_17x33_three_444_ri2', 'mixed_40x56_random_420'):
        case = cases.by_name(name)
        r = cases.reference(case)
        for data, tables, segments in zip(r.files, r.tables, r.segments):
            pieces = jh.jpeg_progressive_pieces(case.h, case.w, case.quality, case.subsampling, tables, qtables=cases.qtables(case),
                                                restart_interval=case.ri)
            assert len(pieces) == 10 and b''.join(p + s for p, s in zip(pieces, segments)) + b'\xff\xd9' == data, name
            assert pieces[0] == jh.jpeg_header(case.h, case.w, case.quality, case.subsampling, huffman=tables, qtables=cases.qtables(case),
                                               restart_interval=case.ri, progressive=True)
            assert pieces[6] == bytes.fromhex('ffda000c' '03' '0100' '0200' '0300' '00' '00' '10')          # no DHT in front of the DC refine scan
            assert jh._jpeg_files(case.h, case.w, case.quality, case.subsampling, [segments], [tables], cases.qtables(case), case.ri, True) == [data]


def test_refusals_and_defaults():
    for fn in (jh.jpeg_header, jh.device_codec, jh.encode_batch, jh.compress_batch, jh.transcode_batch):
        p = inspect.signature(fn).parameters['progressive']
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, fn.__name__
    assert jh.jpeg_header(13, 21, 95, '4:2:0', progressive=False) == jh.jpeg_header(13, 21, 95, '4:2:0') == ref.header(13, 21, 95, 2, 2)
    for bad in (None, oref.ANNEX_K, np.zeros((10, 272), np.int32), np.zeros((10, 271), np.uint8)):
        with pytest.raises(ValueError, match='progressive file'):
            jh.jpeg_header(13, 21, 95, '4:2:0', huffman=bad, progressive=True)
    tables = cases.reference(cases.by_name('g_smooth_8x8_q50_444')).tables[0]
    with pytest.raises(ValueError):
        jh.jpeg_progressive_pieces(8, 8, 50, '4:1:1', tables)
    with pytest.raises(ValueError):
        jh.jpeg_progressive_pieces(8, 8, 50, '4:4:4', tables, restart_interval=65536)
    with pytest.raises(ValueError):
        jh.jpeg_progressive_pieces(8, 8, 50, '4:4:4', tables, qtables=np.ones((2, 64)))        # a quality and tables
    data = cases.golden()['g_smooth_8x8_q50_444'][0]
    with pytest.raises(ValueError):
        jh.parse_header(data)                                                # reading progressive files stays out
    with pytest.raises(ValueError):
        jh.parse_header(data, allow_restart=True)
    assert ops.JPEG_PROGRESSIVE_SCANS == pref.N_SCANS == 10
    assert ops.jpeg_progressive_ecd_bound(16, 16, 1, 1) == 2 * (2 * -(-12 * 27 // 8) + 8 * -(-4 * 1580 // 8))
    assert ops.jpeg_progressive_ecd_bound(16, 16, 2, 2, 1) == ops.jpeg_progressive_ecd_bound(16, 16, 2, 2) + 4 * (4 * 3)
