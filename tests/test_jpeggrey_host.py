"""Grey-scale JPEG files on the host (no GPU): the restatement (tests/jpeggrey_ref.py) against Pillow's files byte
for byte and Pillow's pixels - plain, optimize=True, qtables=, restart intervals, progressive, the factors 2x2 declared -, compression.
jpeg_helpers' header writer and parser with allow_grey and their refusals, the one-component script rules, the geometry helpers against
hand-written values, and the sequential cores of both directions (csrc/jpegd.h, jpegopt.h, jpegrst.h, jpegdprog.h) with the
one-component geometry, built into a stand-alone program under AddressSanitizer and UBSan, on every golden file and on damaged ones."""
import importlib.util
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeggrey_cases as cases
import jpeggrey_ref as gref
from neural_imaging_amd import ops
from neural_imaging_amd.compression import jpeg_helpers as jh

VARIANTS = [(c, v) for c in cases.CASES for v in c.variants]
VARIANT_IDS = ['{}-{}'.format(c.name, v) for c, v in VARIANTS]
OLD_REFUSAL = r'grey-scale file \(3 components needed, the file has 1\)'


def all_files():
    """name -> file: every golden file and the files made in jpeggrey_cases."""
    out = {'{}/{}/{}'.format(c.name, v, i): data for c, v in VARIANTS for i, data in enumerate(cases.golden()[c.name].files[v])}
    out.update({'made/{}/0'.format(tag): v[0] for tag, v in cases.made_here().items()})
    return out


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,variant', VARIANTS, ids=VARIANT_IDS)
def test_restatement_equals_pillow(case, variant):
    g = cases.golden()[case.name]
    assert cases.restated(case, variant)[0] == g.files[variant]
    assert np.array_equal(cases.decoded(case), g.pixels)
    for data, want in zip(g.files[variant], cases.coefficients(case)):           # and back: the parser and the decoder models
        if variant == 'prog':
            flat, status, _ = gref.decode_progressive(data)
            assert status == 0 and np.array_equal(flat, want.reshape(-1))
        else:
            assert np.array_equal(gref.decode_baseline(data), want)


def test_golden_files_are_pillows():
    pytest.importorskip('PIL.Image')
    spec = importlib.util.spec_from_file_location('make_jpeggrey_golden', os.path.join(os.path.dirname(cases.GOLDEN), 'make_jpeggrey_golden.py'))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    for case, variant in VARIANTS:
        g = cases.golden()[case.name]
        for i, img in enumerate(cases.build(case)):
            data, pixels = make.pillow(img, case, variant)
            assert data == g.files[variant][i], (case.name, variant, i)
            assert np.array_equal(pixels, g.pixels[i]), (case.name, variant, i)
    assert os.path.getsize(cases.GOLDEN) < 214364


def test_files_have_the_layout_the_issue_names():
    g = cases.golden()
    small = g['flat+noise+mixed_20x27_q75_ri0'].files
    plain = small['plain'][1]
    assert [plain[k:k + 2] for k in (0, 2, 20, 89, 102, 135, 318)] == [b'\xff\xd8', b'\xff\xe0', b'\xff\xdb', b'\xff\xc0', b'\xff\xc4', b'\xff\xc4',
                                                                     b'\xff\xda']
    assert plain[89:102] == b'\xff\xc0\x00\x0b\x08\x00\x14\x00\x1b\x01\x01\x11\x00' and plain[318:328] == b'\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00'
    assert (gref.HEADER_BYTES, gref.DHT_OFFSET) == (328, 102) == (jh.JPEG_GREY_HEADER_BYTES, jh._GREY_DHT_OFFSET)
    s22 = small['s22'][1]                                     # the factors are declared, the data bytes are the same
    assert s22[:100] == plain[:100] and s22[100] == 0x22 and s22[101:] == plain[101:]
    prog = gref.split(small['prog'][1])
    assert prog['progressive'] and tuple(prog['script']) == gref.SCRIPT_STD and small['prog'][1].count(b'\xff\xc4') >= 5
    marked = g['noise+mixed_20x27_q75_ri5'].files['plain'][0]
    assert marked[318:324] == b'\xff\xdd\x00\x04\x00\x05' and gref.split(marked)['segments'][0].count(b'\xff\xd0') >= 1
    wrapped = gref.split(g['mixed_264x264_q75_ri33'].files['plain'][0])['segments'][0]
    assert gref.markers(264, 264, 33) == 32 and wrapped.count(b'\xff\xd7') == 4
    # flat 4096 blocks: runs of 0x7fff blocks, and refinement scans with nothing to refine
    flat = gref.split(g['flat_512x512_q75_ri0'].files['prog'][0])
    assert [len(s) for s in flat['segments']][1:] == [3, 3, 3, 512, 3] or all(len(s) < 16 for k, s in enumerate(flat['segments']) if k not in (0, 4))
    ids = gref.split(cases.made_here()['ids'][0])
    assert ids['tables'] == gref.split(small['opt'][2])['tables'] and np.array_equal(ids['qtable'], cases.qtable(cases.CASES[2]))
    assert tuple(gref.split(cases.made_here()['bands20x27'][0])['script']) == gref.SCRIPT_BANDS


# ---- 2. the header: written and parsed -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,variant', [(c, v) for c, v in VARIANTS if v in ('plain', 'opt')], ids=[i for i in VARIANT_IDS if i[-4:] != 'prog' and
                                                                                                      i[-3:] != 's22'])
def test_jpeg_header_equals_pillows(case, variant):
    qt = None if not case.qt else cases.QTABLES[case.qt][None]
    tables = cases.restated(case, variant)[1]
    for i, data in enumerate(cases.golden()[case.name].files[variant]):
        head = jh.jpeg_header(case.h, case.w, None if case.qt else case.quality, 'grey', huffman=None if tables is None else tables[i],
                              qtables=qt, restart_interval=case.ri)
        assert head == data[:gref.split(data)['ecd_offset']], (variant, i)
        if variant == 'plain':
            assert len(head) == 328 + (6 if case.ri else 0) and head.index(b'\xff\xc4') == 102


def test_jpeg_header_takes_one_table_or_the_first_of_several():
    arb, ones = cases.QTABLES['arb'], cases.QTABLES['ones']
    one = jh.jpeg_header(20, 27, None, 'grey', qtables=[arb])
    assert one == jh.jpeg_header(20, 27, None, 'grey', qtables=[arb, ones]) == jh.jpeg_header(20, 27, None, 'grey', qtables=[arb, ones, ones])
    assert one == gref.header(20, 27, arb)
    assert jh.check_qtables([arb, ones], grey=True).shape == (1, 64)
    with pytest.raises(ValueError, match='2 tables .luma, chroma. or 3'):
        jh.check_qtables([arb])                               # the colour rule stays
    with pytest.raises(ValueError, match='1 table needed for a grey-scale file'):
        jh.check_qtables([arb] * 4, grey=True)
    with pytest.raises(ValueError, match=r'\(2, 272\) uint8 needed for a grey-scale file'):
        jh.jpeg_header(20, 27, 75, 'grey', huffman=np.zeros((4, 272), np.uint8))
    with pytest.raises(ValueError, match='grey-scale .one-component. images: progressive=True'):
        jh.jpeg_header(20, 27, 75, 'grey', huffman=np.zeros((10, 272), np.uint8), progressive=True)


@pytest.mark.parametrize('name', sorted(all_files()))
def test_parse_header_with_allow_grey(name):
    data = all_files()[name]
    p = gref.split(data)
    hd = jh.parse_header(data, allow_restart=True, allow_progressive=True, allow_grey=True)
    assert len(hd) == 9 and hd.ncomp == 1 and (hd.h, hd.w, hd.hs, hd.vs) == (p['h'], p['w'], 1, 1)          # whatever factors are declared
    assert hd.restart_interval == p['ri'] and hd.qtables.shape == (1, 64) and np.array_equal(hd.qtables[0], p['qtable'])
    assert hd.ecd_offset == p['ecd_offset'] and hd.ecd_end == len(data) - 2
    if p['progressive']:
        assert hd.huffman == () and [s[:5] for s in hd.scans] == p['script']
        assert [list(s.huffman) for s in hd.scans] == p['tables']
        assert [data[s.ecd_offset:s.ecd_end] for s in hd.scans] == p['segments']
        with pytest.raises(ValueError, match='progressive file'):
            jh.parse_header(data, allow_restart=True, allow_grey=True)
    else:
        assert hd.scans == () and list(hd.huffman) == p['tables'][0] and len(hd.huffman) == 2
    # without allow_grey: the old answer, word for word, whatever else is allowed
    for kw in ({}, dict(allow_restart=True, allow_progressive=True)):
        with pytest.raises(ValueError, match='progressive file' if p['progressive'] and not kw else OLD_REFUSAL):
            jh.parse_header(data, **kw)
    for read in (jh.decode_batch, jh.decode_coefficients):
        with pytest.raises(ValueError, match=OLD_REFUSAL):
            read([data], device='no device is touched', allow_restart=True, allow_progressive=True)
    with pytest.raises(ValueError, match=OLD_REFUSAL):
        jh.transcode_batch([data], allow_restart=True, allow_progressive=True)


def test_colour_headers_carry_three_components():
    import jpegrst_cases
    for variant, files in jpegrst_cases.golden()['mixed+noise+smooth_40x56_q75_420_ri5'].files.items():
        hd = jh.parse_header(files[0], allow_restart=True, allow_grey=True)
        old = jh.parse_header(files[0], allow_restart=True)
        assert hd.ncomp == 3 and hd[:4] + hd[5:] == old[:4] + old[5:] and np.array_equal(hd.qtables, old.qtables), variant
        assert hd.qtables.shape == (3, 64) and len(hd.huffman) == 6
    assert jh.JPEGHeader(8, 8, 1, 1, None, (), 0, 0).ncomp == 3 and jh.JPEGHeader(8, 8, 1, 1, None, (), 0, 0).with_scans([]).ncomp == 3
    hd = jh.JPEGHeader(8, 8, 1, 1, None, (), 0, 0).with_ncomp(1).with_scans([1])
    assert hd.ncomp == 1 and hd.scans == (1,) and len(hd) == 9


def test_damaged_grey_headers_are_refused_by_name():
    g = cases.golden()
    base = g['flat+noise+mixed_20x27_q75_ri0'].files['plain'][1]
    marked = g['noise+mixed_20x27_q75_ri5'].files['plain'][0]
    prog = g['flat+noise+mixed_20x27_q75_ri0'].files['prog'][1]
    sos = base.index(b'\xff\xda')
    read = lambda data, **kw: jh.parse_header(data, allow_grey=True, **kw)
    two = base[:sos] + b'\xff\xda\x00\x0a\x02\x01\x00\x02\x00\x00\x3f\x00' + base[sos + 10:]
    with pytest.raises(ValueError, match='the scan holds 2 components, the frame of a grey-scale file one'):
        read(two)
    with pytest.raises(ValueError, match='the scan does not list the components in frame order'):
        read(base[:sos + 5] + b'\x02' + base[sos + 6:])
    with pytest.raises(ValueError, match='missing Huffman table: AC table 1 of component 0'):
        read(base[:sos + 6] + b'\x01' + base[sos + 7:])
    with pytest.raises(ValueError, match='missing Huffman table: DC table 2 of component 0'):
        read(base[:sos + 6] + b'\x20' + base[sos + 7:])
    with pytest.raises(ValueError, match='missing quantisation table 1 of component 0'):
        read(base[:101] + b'\x01' + base[102:])
    with pytest.raises(ValueError, match='malformed SOS segment'):
        read(base[:sos + 2] + b'\x00\x07' + base[sos + 4:sos + 9] + base[sos + 10:])          # a truncated SOS
    with pytest.raises(ValueError, match='truncated'):
        read(base[:sos + 6])
    with pytest.raises(ValueError, match='not a baseline scan'):
        read(base[:sos + 8] + b'\x3e' + base[sos + 9:])
    with pytest.raises(ValueError, match='illegal sampling factors 5x1'):
        read(base[:100] + b'\x51' + base[101:])
    with pytest.raises(ValueError, match='illegal sampling factors 1x0'):
        read(base[:100] + b'\x10' + base[101:])
    for factors in (0x11, 0x12, 0x21, 0x22, 0x41, 0x14, 0x44, 0x33):
        assert read(base[:100] + bytes([factors]) + base[101:])[:4] == (20, 27, 1, 1)
    with pytest.raises(ValueError, match='12-bit samples'):
        read(base[:93] + b'\x0c' + base[94:])
    with pytest.raises(ValueError, match='restart interval 5'):
        read(marked)
    assert read(marked, allow_restart=True).restart_interval == 5
    with pytest.raises(ValueError, match='restart marker FFD0 .* whose restart interval is 0'):
        read(base[:-2] + b'\xff\xd0' + base[-2:], allow_restart=True)
    with pytest.raises(ValueError, match='progressive file'):
        read(prog)
    # CMYK and the rest stay refused, with every keyword
    cmyk = base[:89] + b'\xff\xc0\x00\x14' + base[93:98] + b'\x04' + b'\x01\x11\x00' * 4 + base[102:]
    with pytest.raises(ValueError, match=r'CMYK / four-component file \(3 components needed, the file has 4\)'):
        read(cmyk, allow_restart=True, allow_progressive=True)
    two_comp = base[:89] + b'\xff\xc0\x00\x0e' + base[93:98] + b'\x02' + b'\x01\x11\x00' * 2 + base[102:]
    with pytest.raises(ValueError, match=r'unsupported number of components \(3 components needed, the file has 2\)'):
        read(two_comp)
    # a progressive file: a scan that names the component twice, and one that never finishes
    first = prog.index(b'\xff\xda')
    twice = prog[:first] + b'\xff\xda\x00\x0a\x02\x01\x00\x01\x00\x00\x00\x01' + prog[first + 10:]
    with pytest.raises(ValueError, match='every scan of a one-component frame holds that component, once'):
        read(twice, allow_progressive=True)
    last = prog.rindex(b'\xff\xc4')
    with pytest.raises(ValueError, match='incomplete progression: coefficient 1 of component 0'):
        read(prog[:last] + b'\xff\xd9', allow_progressive=True)


def test_one_component_script_rules():
    assert jh.jpeg_script_check(gref.SCRIPT_STD, 1) == [1, 1, 1, 2, 2, 3] == gref.dpref.levels(gref.SCRIPT_STD)
    assert jh.jpeg_script_check(gref.SCRIPT_BANDS, 1) == [1, 1, 1, 1, 2, 2]
    assert jh.jpeg_script_check([((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 0)], 1) == [1, 1]
    for bad, why in (([((0, 1, 2), 0, 0, 0, 0)], 'one-component frame'), ([((1,), 0, 0, 0, 0)], 'one-component frame'),
                     ([((0, 0), 0, 0, 0, 0)], 'one-component frame'), ([((0,), 1, 63, 0, 0)], 'before the DC first scan'),
                     ([((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1)], 'incomplete progression'), ([((0,), 0, 5, 0, 0)], 'mixes DC and AC'),
                     ([((0,), 0, 0, 0, 0), ((0,), 0, 0, 0, 0)], 'a first scan has Ah = 0'),
                     ([((0,), 0, 0, 0, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 0, 2), ((0,), 1, 63, 2, 0)], 'Al = Ah - 1')):
        with pytest.raises(ValueError, match=why):
            jh.jpeg_script_check(bad, 1)
    # the colour rules are the ones from before: a script of component 0 alone is incomplete there
    with pytest.raises(ValueError, match='incomplete progression: coefficient 0 of component 1'):
        jh.jpeg_script_check(gref.SCRIPT_STD)
    with pytest.raises(ValueError, match='incomplete progression: coefficient 0 of component 1'):
        jh.jpeg_script_check(gref.SCRIPT_STD, 3)


def test_geometry_helpers_against_hand_written_values():
    assert ops.jpeg_subsampling('grey') == ops.JPEG_GREY == (0, 0) and ops.jpeg_is_grey(*ops.JPEG_GREY) and not ops.jpeg_is_grey(1, 1)
    assert ops.jpeg_subsampling('4:2:0') == (2, 2) and ops.jpeg_geometry(20, 27, 1, 1) == (36, 36, [(3, 4)] * 3)          # as before
    assert ops.jpeg_geometry(20, 27, *ops.JPEG_GREY) == (12, 12, [(3, 4)])
    assert ops.jpeg_geometry(1, 1, 0, 0) == (1, 1, [(1, 1)]) and ops.jpeg_geometry(8, 8, 0, 0) == (1, 1, [(1, 1)])
    assert ops.jpeg_geometry(264, 264, 0, 0) == (1089, 1089, [(33, 33)]) and ops.jpeg_geometry(512, 512, 0, 0)[0] == 4096
    assert ops.jpeg_mcu_blocks(0, 0) == 1 and ops.jpeg_mcu_blocks(2, 2) == 6 and ops.jpeg_mcu_blocks(1, 1) == 3
    for ri, markers in ((0, 0), (1, 11), (2, 5), (4, 2), (5, 2), (12, 0), (13, 0), (65535, 0)):            # a restart interval counts blocks
        assert ops.jpeg_restart_markers(20, 27, 0, 0, ri) == markers == gref.markers(20, 27, ri)
        assert ops.jpeg_ecd_bound(20, 27, 0, 0, ri) == 2 * -(-12 * 1658 // 8) + 4 * markers
        assert ops.jpeg_ecd_bound_tables(20, 27, 0, 0, ri) == 2 * -(-12 * 1665 // 8) + 4 * markers
    assert ops.jpeg_restart_markers(40, 56, 2, 2, 5) == 2                                                    # as before
    with pytest.raises(ValueError, match='Unsupported chrominance sub-sampling: gray'):
        ops.jpeg_subsampling('gray')
    for name, args in (('jpeg_progressive_histogram', 3), ('jpeg_encode_progressive', 4), ('jpeg_reconstruct_items', 4), ('jpeg_reconstruct', 4),
                       ('jpeg_transform_items', 2)):
        with pytest.raises(ValueError, match='{}: grey-scale .one-component. batches are not supported here'.format(name)):
            getattr(ops, name)(*([None] * args), hs=0, vs=0)


def test_the_abi_names_one_grey_entry_per_operation():
    from neural_imaging_amd import _lib
    names = {n for n in _lib.PROTOTYPES if n.startswith('nimg_jpeg_grey_')}
    assert names == {'nimg_jpeg_grey_' + n for n in (
        'workspace_bytes', 'transform', 'transform_tables', 'encode', 'histogram', 'encode_tables_workspace_bytes', 'encode_tables',
        'decode_workspace_bytes', 'decode', 'reconstruct_tables', 'decode_progressive_workspace_bytes', 'decode_progressive')}
    assert _lib.ABI_VERSION == 8
    for colour in ('nimg_jpeg_transform', 'nimg_jpeg_encode_restart', 'nimg_jpeg_histogram_restart', 'nimg_jpeg_encode_tables_restart',
                   'nimg_jpeg_decode_restart', 'nimg_jpeg_reconstruct_tables', 'nimg_jpeg_decode_progressive', 'nimg_jpeg_transform_tables'):
        entry, factors = ops._jpeg_entry(colour, 0, 0)
        assert entry in names and factors == () and ops._jpeg_entry(colour, 2, 1) == (colour, (2, 1))
        # the grey form is the colour form without the two factors (and with the interval where the colour form has a twin for it)
        assert len(_lib.PROTOTYPES[entry][1]) == len(_lib.PROTOTYPES[colour][1]) - 2


def test_grey_input_takes_no_chroma_subsampling():
    for shape in ((20, 27, 1), (2, 20, 27, 1)):
        assert jh._grey_input(shape, '4:4:4', 'f') == 'grey' == jh._grey_input(shape, 'grey', 'f')
        with pytest.raises(ValueError, match='grey-scale input .* takes no chroma sub-sampling'):
            jh._grey_input(shape, '4:2:0', 'f')
    assert jh._grey_input((2, 20, 27, 3), '4:2:0', 'f') == '4:2:0'
    with pytest.raises(ValueError, match="subsampling 'grey' needs"):
        jh._grey_input((2, 20, 27, 3), 'grey', 'f')


# ---- 3. the sequential cores under sanitizers, as a stand-alone program -----------------------------------------------------------
@pytest.fixture(scope='module')
def reference():
    try:                                                             # no compiler at all is host_program's assertion: a failure
        cases.host_program(True)
    except subprocess.CalledProcessError as e:
        pytest.fail('the host program does not build with -fsanitize=address,undefined:\n' + e.stdout.decode())
    streams, results, recoded, hists, done = cases.host_reference()
    assert done.returncode == 0 and done.stderr == b'', done.stderr.decode()[-4000:]
    assert len(results) == len(streams) * len(cases.SETTINGS) and len(recoded) == len(streams)
    return streams, results, recoded, hists


def _coefficients_of(name):
    case_name, variant, i = name.split('/')
    if case_name == 'made':
        _, case, i = cases.made_here()[variant]
        return cases.coefficients(case)[i]
    return cases.coefficients(cases.by_name(case_name))[int(i)]


def test_host_program_decodes_and_recodes_every_golden_file(reference):
    streams, results, recoded, hists = reference
    valid = cases.valid_streams()
    assert len(valid) >= 40 and any(s.name == 'made/ids/0' for s in valid)
    for k, s in enumerate(valid):
        want = _coefficients_of(s.name).reshape(-1)
        model = gref.Model(s.h, s.w, [(bytes(t[:16].tolist()), bytes(t[16:].tolist())) for t in s.huffman], s.ecd) if not s.ri and s.h <= 64 \
            else None
        for setting in cases.SETTINGS:
            r = results[(k, setting)]
            assert r.status == 0, (s.name, setting, r.status)
            assert np.array_equal(r.coef, want), (s.name, setting)
            if model:                                       # the restatement's model of the parallel decoder: rounds and subsequences too
                flat, status, rounds, subs = model.run(setting)
                assert (status, rounds, subs) == (0, r.rounds, r.subsequences) and np.array_equal(flat, want), (s.name, setting)
            if setting == 0 and not s.ri:
                assert r.rounds == 0 and r.subsequences == 1
        assert recoded[k] == 1, s.name                      # the writer's core gives the stream back, markers included
        assert np.array_equal(hists[k], gref.histograms(_coefficients_of(s.name), s.ri)), s.name
    big = next(k for k, s in enumerate(valid) if s.name == 'mixed_264x264_q75_ri0/plain/0')
    assert results[(big, 32)].subsequences > 1024 and results[(big, 32)].rounds >= 1
    marked = [k for k, s in enumerate(valid) if s.ri and gref.markers(s.h, s.w, s.ri)]
    assert len(marked) >= 14 and any(results[(k, 2048)].rounds == 0 and results[(k, 2048)].subsequences > 1 for k in marked)


def test_host_program_gives_the_status_the_restatement_predicts_for_damaged_streams(reference):
    streams, results, recoded, _ = reference
    first = len(cases.valid_streams())
    damaged = streams[first:]
    kinds = {s.name.split('|')[1].rstrip('0123456789+-') for s in damaged}
    assert len(damaged) >= 250 and kinds == {'flip', 'truncate', 'renumber', 'remove', 'duplicate', 'dri'}
    bad = 0
    for k, s in enumerate(damaged, first):
        kind = s.name.split('|')[1].rstrip('0123456789+-')
        whole = results[(k, 0)]
        bad += whole.status != 0
        for setting in cases.SETTINGS:
            r = results[(k, setting)]
            assert r.status == whole.status, (s.name, setting)             # the damage reads the same however the stream is cut
            assert r.rounds <= r.subsequences, (s.name, setting)
            if r.status == 0:
                assert np.array_equal(r.coef, whole.coef), (s.name, setting)
        if not s.ri:                                         # without markers the model predicts every status word, and the rounds
            model = gref.Model(s.h, s.w, [(bytes(t[:16].tolist()), bytes(t[16:].tolist())) for t in s.huffman], s.ecd)
            for setting in cases.SETTINGS:
                flat, status, rounds, subs = model.run(setting)
                r = results[(k, setting)]
                assert (status, rounds, subs) == (r.status, r.rounds, r.subsequences), (s.name, setting)
                if status == 0:
                    assert np.array_equal(flat, r.coef), (s.name, setting)
        if kind in ('renumber', 'remove', 'duplicate'):
            assert whole.status & 512, (s.name, whole.status)
        if kind == 'dri':
            assert whole.status & (512 | 32), (s.name, whole.status)
        if kind == 'truncate' and whole.status == 0:         # only padding was cut
            assert recoded[k] in (0, 1)
    assert bad > 120


@pytest.fixture(scope='module')
def progressive_reference():
    names, files, results, done = cases.host_progressive_reference()
    assert done.returncode == 0 and done.stderr == b'', done.stderr.decode()[-4000:]
    assert len(results) == len(files) * len(cases.SETTINGS)
    return names, files, results


def test_host_program_decodes_every_progressive_file(progressive_reference):
    names, files, results = progressive_reference
    valid = [k for k, n in enumerate(names) if '|' not in n]
    assert len(valid) == 7 and sum('made/bands' in names[k] for k in valid) == 2
    for k in valid:
        want = _coefficients_of(names[k]).reshape(-1)
        for setting in cases.SETTINGS:
            r = results[(k, setting)]
            assert r.status == 0 and np.array_equal(r.coef, want), (names[k], setting)
            if len(want) <= 64 * 64:
                flat, status, rounds = gref.decode_progressive(files[k], setting)
                assert status == 0 and rounds == r.rounds and np.array_equal(flat, want), (names[k], setting)
        assert max(results[(k, 0)].rounds) == 0
    noise = names.index('noise_64x64_q75_ri0/prog/0')
    assert max(results[(noise, 32)].rounds) > 1


def test_host_program_gives_the_status_the_restatement_predicts_for_damaged_progressive_files(progressive_reference):
    names, files, results = progressive_reference
    damaged = [k for k, n in enumerate(names) if '|' in n]
    assert len(damaged) >= 25
    bad = 0
    for k in damaged:
        for setting in (32, 0):
            flat, status, rounds = gref.decode_progressive(files[k], setting)
            r = results[(k, setting)]
            assert (status, rounds) == (r.status, r.rounds), (names[k], setting, status, r.status)
            if status == 0:
                assert np.array_equal(flat, r.coef), (names[k], setting)
        bad += results[(k, 0)].status != 0
        assert results[(k, 0)].status == results[(k, 256)].status == results[(k, 2048)].status, names[k]
    assert bad >= 10
