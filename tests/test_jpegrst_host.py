"""JPEG files with restart intervals on the host (no GPU): the restatement (tests/jpegrst_ref.py) against
Pillow's files byte for byte - plain, optimize=True, qtables= -, its parser against the coefficients of the file without markers,
compression.jpeg_helpers' header writer and parser with their refusals, JPEGMarkerStats, a count of the situations the case list
reaches, and the sequential cores of both directions (csrc/jpegd.h, csrc/jpegopt.h, csrc/jpegrst.h) built into a stand-alone program
under AddressSanitizer and UBSan, on every golden file and on a few hundred damaged streams."""
import importlib.util
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_ref as ref
import jpegd_cases
import jpegd_ref as dref
import jpegrst_cases as cases
import jpegrst_ref as rref
from neural_imaging_amd import ops
from neural_imaging_amd.compression import jpeg_helpers as jh

VARIANTS = [(c, v) for c in cases.CASES for v in c.variants]
VARIANT_IDS = ['{}-{}'.format(c.name, v) for c, v in VARIANTS]


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,variant', VARIANTS, ids=VARIANT_IDS)
def test_restatement_equals_pillow(case, variant):
    assert cases.restated(case, variant).files == cases.golden()[case.name].files[variant]


@pytest.mark.parametrize('case', cases.CASES, ids=cases.IDS)
def test_parsed_coefficients_are_those_of_the_file_without_markers(case):
    hs, vs = ref.SUBSAMPLING[case.subsampling]
    g = cases.golden()[case.name]
    for variant in case.variants:
        for i, data in enumerate(g.files[variant]):
            info = rref.parse(data)
            assert info['ri'] == cases.variant_settings(case, variant)[0], (variant, i)
            want = cases.coefficients(case, variant)[i]
            assert all(np.array_equal(a, b) for a, b in zip(info['coefs'], want)), (variant, i)
    if 'base' in case.variants:                       # Pillow's own file without markers, through the parser of jpeg_ref
        for i, data in enumerate(g.files['base']):
            base = dref.real_coefficients(ref.parse(data))
            with_markers = rref.parse(g.files['plain'][i])['coefs']
            assert all(np.array_equal(a, b) for a, b in zip(with_markers, base)), i


def test_golden_files_are_pillows():
    pytest.importorskip('PIL.Image')
    spec = importlib.util.spec_from_file_location('make_jpegrst_golden', os.path.join(os.path.dirname(cases.GOLDEN), 'make_jpegrst_golden.py'))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    for case, variant in VARIANTS:
        g = cases.golden()[case.name]
        for i, img in enumerate(cases.build(case)):
            data, rgb = make.pillow(img, case, variant)
            assert data == g.files[variant][i], (case.name, variant, i)
            if variant == 'plain':
                assert np.array_equal(rgb, g.rgb[i]), (case.name, i)
    assert os.path.getsize(cases.GOLDEN) < 1 << 20


def test_case_list_reaches_every_situation():
    """Counts what the case list reaches, with the restatement's counters and the files themselves."""
    plain = {key: 0 for key in rref.SITUATIONS}
    everything = dict(plain)
    for case, variant in VARIANTS:
        if not variant.startswith('base'):
            for key, n in cases.restated(case, variant).stats.items():
                everything[key] += n
                plain[key] += n if variant == 'plain' else 0
    for key in ('end_aligned', 'end_pad7', 'pad_makes_ff', 'data_ff_before_marker', 'short_last_interval'):
        assert plain[key] >= 1, (key, plain)
    assert all(everything[key] >= 1 for key in rref.SITUATIONS), everything
    # the files agree with the counters: FF 00 FF Dn (a stuffed last byte) occurs, and the marker numbers wrap past D7
    segments = [f[rref.parse(f)['ecd_offset']:-2] for c in cases.CASES for f in cases.golden()[c.name].files['plain']]
    assert any(b'\xff\x00\xff' + bytes([0xd0 + k]) in s for s in segments for k in range(8))
    assert any(b'\xff\xd7' in s and s.count(b'\xff\xd0') >= 2 for s in segments)
    # Ri = one MCU row, the MCU count, more than it, 65535 - on the image with dummy blocks at the right and the bottom
    mcus = {}
    for c in cases.CASES:
        hs, vs = ref.SUBSAMPLING[c.subsampling]
        my, mx = ref.geometry(c.h, c.w, hs, vs)[1]
        mcus.setdefault((c.h, c.w, c.subsampling, my, mx), set()).add(c.ri)
    ris = mcus[(40, 56, '4:2:0', 3, 4)]
    assert {4, 12, 13, 65535} <= ris and any(r % 4 and r < 12 for r in ris)          # 4 = a row; an interval boundary inside a row
    dummies = cases.restated(cases.by_name('mixed+noise+smooth_40x56_q75_420_ri5')).stats
    assert dummies['dummy_right'] and dummies['dummy_bottom'] and dummies['short_last_interval']
    # an optimised DC table that differs from the one of the file without markers
    c = cases.by_name('mixed+noise+smooth_40x56_q75_420_ri5')
    with_markers, without = cases.restated(c, 'opt').huffman, cases.restated(c, 'baseopt').huffman
    assert any(not np.array_equal(a[0], b[0]) or not np.array_equal(a[2], b[2]) for a, b in zip(with_markers, without))


# ---- 2. the header: written and parsed -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,variant', VARIANTS, ids=VARIANT_IDS)
def test_jpeg_header_equals_pillows(case, variant):
    ri, optimize, qt = cases.variant_settings(case, variant)
    for i, data in enumerate(cases.golden()[case.name].files[variant]):
        info = rref.parse(data)
        huffman = cases.restated(case, variant).huffman[i] if optimize else None
        head = jh.jpeg_header(case.h, case.w, None if qt is not None else case.quality, case.subsampling, huffman=huffman, qtables=qt,
                              restart_interval=ri)
        assert head == data[:info['ecd_offset']], (variant, i)
        if ri and not optimize:
            assert len(head) == (629 if qt is None or len(qt) == 2 else 698) and head.index(b'\xff\xc4') == (177 if len(head) == 629 else 246)
            assert head[-20:-14] == b'\xff\xdd\x00\x04' + struct.pack('>H', ri)
            assert head[:-20] + head[-14:] == jh.jpeg_header(case.h, case.w, None if qt is not None else case.quality, case.subsampling,
                                                             qtables=qt)


@pytest.mark.parametrize('value', [-1, 65536, 70000, 1.5, 'four', None, True])
def test_restart_interval_outside_the_range_is_refused(value):
    with pytest.raises(ValueError, match='restart_interval'):
        jh.jpeg_header(16, 16, 75, restart_interval=value)
    with pytest.raises(ValueError, match='restart_interval'):
        ops.jpeg_restart_interval(value)


def test_restart_interval_zero_is_todays_header_and_bounds():
    assert jh.jpeg_header(40, 56, 75, '4:2:0', restart_interval=0) == jh.jpeg_header(40, 56, 75, '4:2:0')
    assert ops.jpeg_ecd_bound(40, 56, 2, 2, 0) == ops.jpeg_ecd_bound(40, 56, 2, 2)
    for ri, markers in ((1, 11), (4, 2), (5, 2), (12, 0), (13, 0), (65535, 0)):
        assert ops.jpeg_restart_markers(40, 56, 2, 2, ri) == markers == rref.markers(40, 56, 2, 2, ri)
        assert ops.jpeg_ecd_bound(40, 56, 2, 2, ri) == ops.jpeg_ecd_bound(40, 56, 2, 2) + 4 * markers
        assert ops.jpeg_ecd_bound_tables(40, 56, 2, 2, ri) == ops.jpeg_ecd_bound_tables(40, 56, 2, 2) + 4 * markers


@pytest.mark.parametrize('case,variant', VARIANTS, ids=VARIANT_IDS)
def test_parse_header_with_allow_restart(case, variant):
    for data in cases.golden()[case.name].files[variant]:
        hd, info, head = jh.parse_header(data, allow_restart=True), rref.parse(data), dref.header(data)
        assert (hd.h, hd.w, hd.hs, hd.vs) == (info['h'], info['w'], info['hs'], info['vs'])
        assert hd.restart_interval == info['ri'] == cases.variant_settings(case, variant)[0]
        assert (hd.ecd_offset, hd.ecd_end) == (info['ecd_offset'], len(data) - 2)
        assert np.array_equal(hd.qtables, info['qtables']) and list(hd.huffman) == head['tables']
        assert jh.parse_header(data, True)[-1] == hd[8] == hd.restart_interval and len(hd) == 9      # positional, the trailing field
        if info['ri']:
            with pytest.raises(ValueError, match='restart interval'):
                jh.parse_header(data)
        else:
            assert jh.parse_header(data).restart_interval == 0


def test_parse_header_refusals_with_allow_restart():
    g = cases.golden()[cases.by_name('mixed+noise+smooth_40x56_q75_420_ri5').name]
    with_markers, without = g.files['plain'][0], g.files['base'][0]
    sos = with_markers.index(b'\xff\xda')
    # a restart marker in a file whose interval is 0: no DRI segment, and a DRI segment of 0
    stray = without[:-2] + b'\xff\xd0' + without[-2:]
    zero = with_markers[:sos - 2] + b'\x00\x00' + with_markers[sos:]
    for data in (stray, zero):
        with pytest.raises(ValueError, match='restart marker FFD0 .* whose restart interval is 0'):
            jh.parse_header(data, allow_restart=True)
        with pytest.raises(ValueError, match='restart marker'):
            jh.decode_batch([data], device='no device is touched', allow_restart=True)
    with pytest.raises(ValueError, match='restart marker'):                          # the default's message stays
        jh.parse_header(stray)
    # several DRI segments: equal values are one interval, different ones are refused by name
    twice = with_markers[:sos] + b'\xff\xdd\x00\x04\x00\x05' + with_markers[sos:]
    assert jh.parse_header(twice, allow_restart=True).restart_interval == 5
    differ = with_markers[:sos] + b'\xff\xdd\x00\x04\x00\x04' + with_markers[sos:]
    with pytest.raises(ValueError, match='several DRI segments with different restart intervals .5 and 4'):
        jh.parse_header(differ, allow_restart=True)
    with pytest.raises(ValueError, match='several DRI segments'):
        jh.transcode_batch([differ], allow_restart=True)
    with pytest.raises(ValueError, match='malformed DRI'):
        jh.parse_header(with_markers[:sos - 4] + b'\x00\x05\x00\x05\x00' + with_markers[sos:], allow_restart=True)
    # without the keyword every reader refuses before a device is touched
    for read in (jh.decode_batch, jh.decode_coefficients):
        with pytest.raises(ValueError, match='restart interval'):
            read([with_markers], device='no device is touched')
    with pytest.raises(ValueError, match='restart interval'):
        jh.transcode_batch([with_markers])
    assert 512 in jh.JPEG_STATUS_BITS and 'restart markers' in jh.JPEG_STATUS_BITS[512]


def test_marker_stats_parses_restart_files():
    """The reference's behaviour: 'RST' is the offset of the DRI segment; the effective size counts from the first Huffman table."""
    for case, variant in VARIANTS:
        ri = cases.variant_settings(case, variant)[0]
        for data in cases.golden()[case.name].files[variant]:
            stats = jh.JPEGMarkerStats(data)
            assert stats.shape == (case.h, case.w, 3) and stats.get_bytes() == len(data)
            assert stats.get_effective_bytes() == len(data) - data.index(b'\xff\xc4')
            assert ('RST' in stats.blocks) == bool(ri)
            if ri:
                assert data[stats.blocks['RST']:stats.blocks['RST'] + 6] == b'\xff\xdd\x00\x04' + struct.pack('>H', ri)
                assert stats.blocks['RST'] + 6 == stats.blocks['SOS']


# ---- 3. the sequential cores under sanitizers, as a stand-alone program -----------------------------------------------------------
@pytest.fixture(scope='module')
def reference():
    try:                                                             # no compiler at all is host_program's assertion: a failure
        cases.host_program(True)
    except subprocess.CalledProcessError as e:
        pytest.fail('the host program does not build with -fsanitize=address,undefined:\n' + e.stdout.decode())
    streams, results, recoded, done = cases.host_reference()
    assert done.returncode == 0 and done.stderr == b'', done.stderr.decode()[-4000:]
    assert len(results) == len(streams) * len(cases.SETTINGS) and len(recoded) == len(streams)
    lines = done.stdout.decode().splitlines()
    assert len(lines) == len(results) and all('coefficients' in ln and 'rounds' in ln and 'status' in ln for ln in lines)
    return streams, results, recoded


def test_existing_host_programs_build_untouched():
    """tests/jpegd_host.cpp and tests/jpegopt_host.cpp include the headers this feature extends."""
    import jpegopt_cases
    assert os.path.exists(jpegd_cases.host_program(False)) and os.path.exists(jpegopt_cases.host_program(False))


def test_host_program_decodes_and_recodes_every_golden_file(reference):
    streams, results, recoded = reference
    valid = cases.valid_streams()
    assert set(cases.SETTINGS) >= {32, 256, 2048}
    for k, s in enumerate(valid):
        name, variant, i = s.name.split('/')
        want = ref.flat_coefficients(cases.coefficients(cases.by_name(name), variant)[int(i)])
        for setting in cases.SETTINGS:
            r = results[(k, setting)]
            assert r.status == 0, (s.name, setting, r.status)
            assert np.array_equal(r.coef, want), (s.name, setting)
            # every interval is an entry point: its first subsequence is true before round 0
            longest = max(-(-len(p) * 8 // setting) if setting else 1 for p in rref.split_segment(s.ecd)[0])
            assert r.rounds <= max(longest - 1, 0), (s.name, setting, r.rounds, longest)
            if setting == 0 or longest <= 1:
                assert r.rounds == 0, (s.name, setting)
        assert recoded[k] == 1, s.name                     # the writer's core gives the stream back, markers included
    with_markers = [k for k, s in enumerate(valid) if s.ri and rref.markers(s.h, s.w, s.hs, s.vs, s.ri)]
    assert len(with_markers) > 50 and any(results[(k, 32)].rounds > 100 for k in with_markers)
    assert any(results[(k, 2048)].rounds == 0 and results[(k, 2048)].subsequences > 1 for k in with_markers)


def test_host_program_without_an_interval_is_the_decoder_of_section_4e(reference):
    """Ri = 0 through the interval-aware steps = tests/jpegd_host.cpp, status, rounds, subsequences and coefficients."""
    streams, results, _ = reference
    plain = [(k, s) for k, s in enumerate(cases.valid_streams()) if s.ri == 0]
    assert len(plain) >= 8
    old, done = jpegd_cases.host_results([jpegd_cases.Stream(s.name, s.h, s.w, s.hs, s.vs, s.huffman, s.ecd) for _, s in plain],
                                         settings=cases.SETTINGS, sanitize=False)
    assert done.returncode == 0
    for j, (k, s) in enumerate(plain):
        for setting in cases.SETTINGS:
            a, b = results[(k, setting)], old[(j, setting)]
            assert (a.status, a.rounds, a.subsequences) == (b.status, b.rounds, b.subsequences), (s.name, setting)
            assert np.array_equal(a.coef, b.coef), (s.name, setting)


def test_host_program_survives_damaged_streams(reference):
    streams, results, recoded = reference
    first = len(cases.valid_streams())
    damaged = streams[first:]
    kinds = [s.name.split('|')[1].rstrip('0123456789+-') for s in damaged]
    assert len(damaged) >= 300 and {'renumber', 'remove', 'duplicate', 'truncate', 'flip', 'stray', 'dri'} == set(kinds)
    for k, s in enumerate(damaged, first):
        kind = s.name.split('|')[1].rstrip('0123456789+-')
        whole = results[(k, 0)]
        for setting in cases.SETTINGS:
            r = results[(k, setting)]
            assert r.status == whole.status, (s.name, setting)             # the damage reads the same however the stream is cut
            assert r.rounds <= r.subsequences, (s.name, setting)
            if r.status == 0:
                assert np.array_equal(r.coef, whole.coef), (s.name, setting)
        if kind in ('renumber', 'remove', 'duplicate'):
            assert whole.status & 512, (s.name, whole.status)
        if kind == 'dri' and '|dri0' not in s.name:
            assert whole.status & (512 | 32), (s.name, whole.status)
        if '|dri0' in s.name:
            assert whole.status & 1 and not whole.status & 512, (s.name, whole.status)       # markers like any other
        if kind == 'stray':                                # what stands between the last block and the marker is skipped
            original = next(v for v in cases.valid_streams() if v.name == s.name.split('|')[0])
            j = cases.valid_streams().index(original)
            assert whole.status == 0 and np.array_equal(whole.coef, results[(j, 0)].coef), s.name
        if kind == 'truncate' and whole.status == 0:       # only padding was cut
            assert recoded[k] in (0, 1)
    assert sum(results[(k, 0)].status != 0 for k in range(first, len(streams))) > 150
