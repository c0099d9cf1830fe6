"""Optimised Huffman tables on the host (no GPU): the plain Python restatement (tests/jpegopt_ref.py) against Pillow's optimize=True
and the committed golden files, what the case list reaches, the sequential core of csrc/jpegopt.h built into a stand-alone program
under AddressSanitizer and UBSan against the restatement, and the host half of the product (jpeg_header(huffman=...), JPEGMarkerStats
and parse_header on an optimised file)."""
import importlib.util
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_cases
import jpeg_ref as ref
import jpegopt_cases as cases
import jpegopt_ref as oref
from neural_imaging_amd.compression import jpeg_helpers as jh


def _pillow(img, quality, subsampling):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format='JPEG', quality=quality, subsampling=jpeg_cases.SUBSAMPLINGS.index(subsampling), optimize=True)
    return buf.getvalue()


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------
def test_restatement_equals_pillow():
    """Whole files, every case, the length-limiting image included."""
    pytest.importorskip('PIL.Image')
    for case in cases.CASES:
        r = cases.reference(case)
        for i, img in enumerate(cases.build(case)):
            assert r.files[i] == _pillow(img, case.quality, case.subsampling), (case.name, i)


def test_restatement_equals_golden():
    golden = cases.golden()
    assert sorted(golden) == sorted(c.name for c in jpeg_cases.GOLDEN_CASES)
    for case in jpeg_cases.GOLDEN_CASES:
        assert golden[case.name] == cases.reference(case).files, case.name


def test_golden_files_are_pillows():
    pytest.importorskip('PIL.Image')
    spec = importlib.util.spec_from_file_location('make_jpegopt_golden', os.path.join(os.path.dirname(cases.GOLDEN), 'make_jpegopt_golden.py'))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    golden = cases.golden()
    for case in jpeg_cases.GOLDEN_CASES:
        assert golden[case.name] == [make.pillow(img, case.quality, case.subsampling) for img in jpeg_cases.build(case)], case.name
    assert os.path.getsize(cases.GOLDEN) < os.path.getsize(jpeg_cases.GOLDEN)


def test_optimised_files_decode_to_the_same_coefficients():
    """The restatement's parser finds the encoder's coefficients behind the optimised tables, and the files are the smaller ones."""
    for case in jpeg_cases.GOLDEN_CASES[::5] + [cases.LIMITED]:
        r = cases.reference(case)
        for i, data in enumerate(r.files):
            parsed = ref.parse(data)
            for k, c in enumerate(r.coefs[i]):
                assert np.array_equal(parsed['coefs'][k][:c.shape[0], :c.shape[1]], c), (case.name, k)
            assert np.array_equal(oref.tables_of_file(data), r.tables[i]), case.name
            if case is not cases.LIMITED:
                assert len(data) < len(jpeg_cases.reference(case).files[i]), case.name


def test_case_list_reaches_every_path():
    """A case list that no longer reaches a path of the table construction must say so."""
    limited = single = zrl = 0
    kinds = set()
    for case in cases.CASES:
        r = cases.reference(case)
        hs, vs = ref.SUBSAMPLING[case.subsampling]
        for i in range(len(r.files)):
            for t in range(4):
                limited += max(oref.code_sizes(r.hists[i, t])[:256]) > 16
                single += int(r.tables[i, t, :16].sum()) == 1
            zrl += int(r.hists[i, 1, 0xf0]) + int(r.hists[i, 3, 0xf0])
            if case.h <= 64:
                kinds |= {s[4] for s in oref.block_symbols(r.coefs[i], case.h, case.w, hs, vs)}
    assert limited >= 1 and single >= 1 and zrl >= 1
    assert {'right', 'bottom'} <= kinds
    r = cases.reference(cases.LIMITED)
    assert max(oref.code_sizes(r.hists[0, 3])[:256]) == 17 and len(r.files[0]) == 51971
    names, hists = cases.synthetic()
    tables, status = cases.synthetic_reference()
    want = {'fibonacci-20': 20, 'fibonacci-24': 24, 'fibonacci-30': 30, 'fibonacci-40': 40, 'single': 1, 'two-equal': 2}
    for name, size in want.items():
        assert max(oref.code_sizes(hists[names.index(name)])) == size, name
    assert status[names.index('fibonacci-40')] == oref.ST_OVERFLOW and not tables[names.index('fibonacci-40')].any()
    assert [int(status[names.index(n)]) for n in ('total-2^32', 'total-2^32-1', 'total-2^32-2')] == [oref.ST_TOTAL, oref.ST_TOTAL, 0]
    assert status[names.index('zeros')] == 0 and not tables[names.index('zeros')].any()
    assert tables[names.index('two-equal'), 16:18].tolist() == [3, 200]          # the tie: 200, the larger index, merges with the pseudo-symbol
    assert len(names) == 211 and int((status != 0).sum()) == 3


# ---- 2. the sequential core under sanitizers, as a stand-alone program --------------------------------------------------------
@pytest.fixture(scope='module')
def host():
    try:
        cases.host_program(True)
    except subprocess.CalledProcessError as e:
        pytest.fail('the host program does not build with -fsanitize=address,undefined:\n' + e.stdout.decode())
    images, refs = [], []
    for case in jpeg_cases.GOLDEN_CASES:
        r = cases.reference(case)
        hs, vs = ref.SUBSAMPLING[case.subsampling]
        for i in range(len(r.files)):
            images.append(cases.Image(case.h, case.w, hs, vs, r.flat[i]))
            refs.append((case.name, r.hists[i], r.tables[i]))
    given = [oref.ANNEX_K] + _given_tables()
    tables, status, out, derived, done = cases.host_results(cases.synthetic()[1], images, given, sanitize=True)
    assert done.returncode == 0 and done.stderr == b'', done.stderr.decode()[-4000:]
    return tables, status, out, derived, refs, given


def _given_tables():
    """Table sets the derive step must refuse or survive: too many codes of a length, more than 256 symbols, symbols listed twice, a DC
    table with symbols above 15, all zeros."""
    out = []
    for t, length, count in ((0, 0, 3), (1, 1, 5), (3, 15, 255), (2, 7, 255)):
        bad = oref.ANNEX_K.copy()
        bad[t, length] = count
        out.append(bad)
    twice = oref.ANNEX_K.copy()
    twice[1, 16:20] = 0x11
    out.append(twice)
    dc = oref.ANNEX_K.copy()
    dc[0, 16:28] = np.arange(12) * 20
    out.append(dc)
    out.append(np.zeros((4, 272), np.uint8))
    full = np.zeros((4, 272), np.uint8)                 # 256 symbols: every byte of the table in use
    full[:, 7] = 255
    full[:, 8] = 1
    full[:, 16:] = np.arange(256)
    out.append(full)
    return out


def test_host_program_builds_the_restatements_tables(host):
    tables, status, _, _, _, _ = host
    want_tables, want_status = cases.synthetic_reference()
    names = cases.synthetic()[0]
    for k, name in enumerate(names):
        assert status[k] == want_status[k] and np.array_equal(tables[k], want_tables[k]), name


def test_host_program_counts_and_derives_as_the_restatement(host):
    _, _, out, derived, refs, given = host
    assert len(out) == len(refs)
    for o, (name, hist, tables) in zip(out, refs):
        assert np.array_equal(o.hist, hist), name
        assert np.array_equal(o.tables, tables) and not o.status.any(), name
        valid, codes = cases.code_words(tables)
        assert o.valid == valid == 1 and np.array_equal(o.codes, codes), name
    verdicts = []
    for (valid, codes), tables in zip(derived, given):
        want_valid, want = cases.code_words(tables)
        assert valid == want_valid and np.array_equal(codes, want)
        verdicts.append(valid)
    assert verdicts == [1, 0, 0, 0, 0, 1, 1, 1, 1]


# ---- 3. the host half of the product --------------------------------------------------------------------------------------------
def test_header_and_marker_stats_on_optimised_files():
    for case in (jpeg_cases.by_name('smooth+noise+half_13x21_q95_420'), jpeg_cases.by_name('constant_16x16_q75_444'), cases.LIMITED):
        r = cases.reference(case)
        hs, vs = ref.SUBSAMPLING[case.subsampling]
        for i, data in enumerate(r.files):
            head = jh.jpeg_header(case.h, case.w, case.quality, case.subsampling, huffman=r.tables[i])
            assert head == oref.header(case.h, case.w, case.quality, hs, vs, r.tables[i]) and data.startswith(head)
            counted, = jh._header_lengths(case.h, case.w, case.quality, case.subsampling, 1, np.asarray(r.tables[i])[None], None, 0, False)
            assert len(head) == int(counted) == len(data) - len(r.ecds[i]) - 2
            stats = jh.JPEGMarkerStats(data)
            assert stats.blocks['DHT:0'] == 177 and stats.blocks['ECD'] == len(head) and stats.get_bytes() == len(data)
            assert stats.get_effective_bytes() == len(data) - 177 and stats.shape == (case.h, case.w, 3)
            at = 177
            for ident, t in zip(oref.TABLE_IDS, r.tables[i]):
                assert stats.blocks['DHT:{}'.format(ident)] == at
                at += 21 + int(t[:16].sum())
            assert stats.blocks['SOS'] == at
            hd = jh.parse_header(data)
            assert (hd.h, hd.w, hd.hs, hd.vs, hd.ecd_offset, hd.ecd_end) == (case.h, case.w, hs, vs, len(head), len(data) - 2)
            for k, (counts, symbols) in enumerate(hd.huffman):
                t = r.tables[i][k if k < 4 else k - 2]
                assert counts == t[:16].tobytes() and symbols == t[16:16 + len(symbols)].tobytes()
    assert jh.jpeg_header(13, 21, 95, '4:2:0', huffman=oref.ANNEX_K) == jh.jpeg_header(13, 21, 95, '4:2:0') == ref.header(13, 21, 95, 2, 2)
    with pytest.raises(ValueError):
        jh.jpeg_header(13, 21, 95, huffman=np.zeros((6, 272), np.uint8))
