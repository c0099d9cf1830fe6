"""The samplings 4:4:0, 4:1:1, 4:1:0, 1x4 and 2x4 on the host (no GPU): the restatement (tests/jpegsamp_ref.py)
against the pixels Pillow decodes at every scale it can be asked for, parse_header's allow_sampling and its refusals, the refusals of
what is out of scope, and the sequential cores (csrc/jpeg_geo.h, jpegd.h, jpegopt.h, jpegrst.h, jpegdprog.h, jpegscale.h) built with the
wide set of factors into stand-alone programs under AddressSanitizer and UBSan, run on every golden file and on damaged copies."""
import importlib.util
import os

import numpy as np
import pytest

import jpeg_ref as ref
import jpegdprog_ref as dprog
import jpegrst_ref as rref
import jpegsamp_cases as cases
import jpegsamp_ref as sr
from neural_imaging_amd import ops
from neural_imaging_amd.compression import jpeg_helpers as jh

ALLOW = dict(allow_restart=True, allow_progressive=True, allow_sampling=True)
ALL_EIGHT = sorted(sr.SAMPLINGS.values())


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', cases.CASES, ids=cases.IDS)
def test_restatement_equals_pillow(case):
    g = cases.golden()[case.name]
    asked = [s for s in cases.SCALES if cases.askable(case, s)]
    assert sorted(g.crcs) == asked and sorted(g.pixels) == [s for s in asked if cases.pixels_held(case, s)]
    for s in asked:
        got = cases.expected(case, s)
        assert got.shape == (-(-case.h // s), -(-case.w // s), 3)
        assert cases.crc(got) == g.crcs[s], (case.name, s)
        if s in g.pixels:
            assert np.array_equal(got, g.pixels[s]), (case.name, s)
    for variant in case.variants:                                    # the files are the test writer's: its coefficients are theirs
        assert g.files[variant] == cases.written(case, variant), (case.name, variant)


def test_no_case_is_left_out():
    assert {c.sampling for c in cases.CASES} == set(sr.WIDE) and sorted(cases.golden()) == sorted(cases.IDS)
    for sampling, (hs, vs) in sr.WIDE.items():
        mine = [c for c in cases.CASES if c.sampling == sampling]
        sizes = {(c.h, c.w) for c in mine}
        assert {(1, 1), (8, 8), (8 * vs, 8 * hs), (16 * vs, 8 * hs), (17, 33), (33, 17), cases.VARIED} <= sizes
        chroma = {(-(-h // vs), -(-w // hs)) for h, w in sizes}
        assert {(3, 1), (1, 2), (3, 3)} <= chroma                     # one and two columns, one row, and a width past the `> 2`
        varied = [c for c in mine if (c.h, c.w) == cases.VARIED]
        assert {(c.content, c.quality) for c in varied} == {('noise', 30), ('mixed', 90)}
        assert [c.variants for c in varied if c.quality == 90] == [cases.VARIANTS]
    # 4:1:0: a scaled chroma row of 2 | 3 samples at 1/2 and at 1/4, where h2v1 turns from replication to the triangle filter
    for s, widths in ((2, (8, 9)), (4, (16, 17))):
        assert [sr.scaled_geometry(16, w, 4, 2, s)['mode'] for w in widths] == ['replicate', 'h2v1']
        assert {(16, w) for w in widths} <= {(c.h, c.w) for c in cases.CASES if c.sampling == '4:1:0'}


def test_golden_file_is_pillows():
    pytest.importorskip('PIL.Image')
    spec = importlib.util.spec_from_file_location('make_jpegsamp_golden', os.path.join(os.path.dirname(cases.GOLDEN), 'make_jpegsamp_golden.py'))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    g = cases.golden()
    for case in cases.CASES:
        for variant in case.variants:
            for s in cases.SCALES:
                if cases.askable(case, s):
                    scale, px = make.draft(g[case.name].files[variant], None if s == 1 else cases.request(case, s))
                    assert scale == s and cases.crc(px) == g[case.name].crcs[s], (case.name, variant, s)


def test_upsampler_table():
    """The up-sampler per sampling x scale as DESIGN.md section 4r states it (rows wide enough for the triangle filters)."""
    want = {(1, 2): ('h1v2', 'h1v2', 'h1v2', 'replicate'), (4, 1): ('replicate',) * 4, (1, 4): ('replicate',) * 4,
            (4, 2): ('replicate', 'h2v1', 'h2v1', 'replicate'), (2, 4): ('replicate', 'h1v2', 'h1v2', 'replicate'),
            (1, 1): ('none',) * 4, (2, 1): ('h2v1', 'h2v1', 'h2v1', 'replicate'), (2, 2): ('h2v2', 'none', 'none', 'none')}
    blocks = {(1, 2): (8, 4, 2, 1), (4, 1): (8, 4, 2, 1), (1, 4): (8, 4, 2, 1), (4, 2): (8, 8, 4, 2), (2, 4): (8, 8, 4, 2),
              (1, 1): (8, 4, 2, 1), (2, 1): (8, 4, 2, 1), (2, 2): (8, 8, 4, 2)}
    for (hs, vs), modes in want.items():
        got = [sr.scaled_geometry(128, 128, hs, vs, s) for s in cases.SCALES]
        assert tuple(g['mode'] for g in got) == modes, (hs, vs)
        assert tuple(g['nC'] for g in got) == blocks[(hs, vs)] and tuple(g['nY'] for g in got) == (8, 4, 2, 1), (hs, vs)
    assert [sr.scaled_geometry(16, 16, 4, 2, 2)[k] for k in ('nC', 'rx', 'ry')] == [8, 2, 1]          # the issue's examples
    assert [sr.scaled_geometry(16, 16, 1, 2, 2)[k] for k in ('nC', 'rx', 'ry')] == [4, 1, 2]
    assert [sr.scaled_geometry(16, 16, 4, 1, 2)[k] for k in ('nC', 'rx', 'ry', 'mode')] == [4, 4, 1, 'replicate']


# ---- 2. the header ------------------------------------------------------------------------------------------------------------
def _with_sampling(data, luma, cb=0x11, cr=0x11):
    """The file with other sampling bytes in its frame header (the scan no longer fits: parse_header does not decode)."""
    at = data.index(b'\xff\xc0') if b'\xff\xc0' in data else data.index(b'\xff\xc2')
    out = bytearray(data)
    out[at + 11], out[at + 14], out[at + 17] = luma, cb, cr
    return bytes(out)


@pytest.mark.parametrize('case', [c for c in cases.CASES if (c.h, c.w) == cases.VARIED and c.quality == 90], ids=lambda c: c.sampling)
def test_parse_header(case):
    hs, vs = cases.factors(case)
    for variant, data in cases.golden()[case.name].files.items():
        with pytest.raises(ValueError, match=r'unsupported sampling factors {}x{} 1x1 1x1 \(luma 1x1, 2x1 or 2x2 over 1x1 chroma\)'.format(hs, vs)):
            jh.parse_header(data, allow_restart=True, allow_progressive=True)
        hd = jh.parse_header(data, **ALLOW)
        assert (hd.h, hd.w, hd.hs, hd.vs, hd.ncomp) == (case.h, case.w, hs, vs, 3)
        assert hd.restart_interval == cases.restart_interval(case, variant) and bool(hd.scans) == variant.startswith('prog')
        assert np.array_equal(hd.qtables, cases.table_words(case))
    plain = cases.golden()[case.name].files['plain']
    if case.sampling != '4:4:0':
        return
    for luma, cb, cr in ((0x31, 0x11, 0x11), (0x13, 0x11, 0x11), (0x44, 0x11, 0x11), (0x33, 0x11, 0x11), (0x24, 0x12, 0x12),
                         (0x22, 0x21, 0x21), (0x12, 0x11, 0x12), (0x21, 0x12, 0x12), (0x41, 0x21, 0x21)):
        named = '{}x{} {}x{} {}x{}'.format(luma >> 4, luma & 15, cb >> 4, cb & 15, cr >> 4, cr & 15)
        with pytest.raises(ValueError, match='unsupported sampling factors {} .*1x2, 4x1, 4x2, 1x4 or 2x4 over 1x1 chroma'.format(named)):
            jh.parse_header(_with_sampling(plain, luma, cb, cr), allow_sampling=True)
        with pytest.raises(ValueError, match=r'unsupported sampling factors {} \(luma 1x1, 2x1 or 2x2 over 1x1 chroma\)'.format(named)):
            jh.parse_header(_with_sampling(plain, luma, cb, cr))
    for luma in (0x11, 0x21, 0x22):                                   # the three, with and without the keyword: what they were
        a, b = jh.parse_header(_with_sampling(plain, luma)), jh.parse_header(_with_sampling(plain, luma), allow_sampling=True)
        assert a[:4] == b[:4] == (case.h, case.w, luma >> 4, luma & 15)


def test_out_of_scope_is_refused_by_name():
    x = np.zeros((1, 16, 16, 3), np.uint8)
    for name in sr.WIDE:
        with pytest.raises(ValueError, match='Unsupported chrominance sub-sampling: {} .*read and transcoded .*not written from pixels'.format(name)):
            ops.jpeg_subsampling(name)
        for call in (lambda: jh.encode_batch(x, 75, name), lambda: jh.compress_batch(x, 75, subsampling=name),
                     lambda: jh.rate_distortion(x, [50], name), lambda: jh.match_quality_batch(x, subsampling=name)):
            with pytest.raises(ValueError, match='not written from pixels'):
                call()
    with pytest.raises(ValueError, match='Unsupported chrominance sub-sampling: 4:1:2 \\(4:4:4, 4:2:2 or 4:2:0\\)$'):
        ops.jpeg_subsampling('4:1:2')
    for hs, vs in sr.WIDE.values():
        assert ops.jpeg_is_wide(hs, vs) and not ops.jpeg_is_grey(hs, vs)
        for entry in ('nimg_jpeg_transform', 'nimg_jpeg_encode_restart', 'nimg_jpeg_transform_tables', 'nimg_jpeg_encode_progressive',
                      'nimg_jpeg_progressive_histogram'):
            with pytest.raises(ValueError, match='the sampling factors {}x{} are only read from files'.format(hs, vs)):
                ops._jpeg_entry(entry, hs, vs)
        assert ops._jpeg_entry('nimg_jpeg_decode_restart', hs, vs) == ('nimg_jpeg_sampling_decode', (hs, vs))
        assert ops._jpeg_entry('nimg_jpeg_workspace_bytes', hs, vs, 0) == ('nimg_jpeg_sampling_reconstruct_scaled_workspace_bytes', (hs, vs, 1))
    for hs, vs in sr.THREE.values():
        assert not ops.jpeg_is_wide(hs, vs) and ops._jpeg_entry('nimg_jpeg_decode_restart', hs, vs) == ('nimg_jpeg_decode_restart', (hs, vs))


def test_new_entries_are_declared():
    from neural_imaging_amd import _lib
    new = {n for n in _lib.PROTOTYPES if n.startswith('nimg_jpeg_sampling_')}
    assert new == set(ops._JPEG_SAMPLING_ENTRIES.values()) and len(new) == 10
    for old, name in ops._JPEG_SAMPLING_ENTRIES.items():             # the arguments and the result of the namesake
        assert _lib.PROTOTYPES[name] == _lib.PROTOTYPES[old], name
        assert hasattr(_lib.load(), name)
    assert _lib.ABI_VERSION == 8


# ---- 3. the cores under the sanitizers ------------------------------------------------------------------------------------------
def test_host_geometry():
    queries = [(c.h, c.w) + cases.factors(c) for c in cases.CASES] + [(37, 67, hs, vs) for hs, vs in sr.THREE.values()]
    refused = [(16, 16, hs, vs) for hs, vs in ((3, 1), (1, 3), (4, 4), (4, 3), (2, 3), (0, 1), (8, 1), (1, 8))]
    got, done = cases.host_geometry(queries + refused)
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    for (h, w, hs, vs), (three, wide, geo, scaled) in zip(queries, got):
        assert wide and three == ((hs, vs) in sr.THREE.values()), (hs, vs)               # the default set refuses what it refused
        want = sr.geometry(h, w, hs, vs)
        assert {k: geo[k] for k in want} == want and 1 << geo['hsh'] == hs, (h, w, hs, vs)
        assert (geo['NB'], geo['SB']) == ops.jpeg_geometry(h, w, hs, vs)[:2]
        for s in cases.REDUCED:
            sg = sr.scaled_geometry(h, w, hs, vs, s)
            if sg['mode'] == 'h2v2':                                  # (never over 1x1 chroma at a reduced scale)
                assert not scaled[s]['ok']
                continue
            assert scaled[s]['ok'] == 1
            assert {k: scaled[s][k] for k in sg if k != 'mode'} == {k: v for k, v in sg.items() if k != 'mode'}, (h, w, hs, vs, s)
            assert scaled[s]['mode'] == cases.MODES[sg['mode']], (h, w, hs, vs, s)
    assert all(not three and not wide for three, wide, _, _ in got[len(queries):])
    assert not any(sr.scaled_geometry(64, 64, hs, vs, s)['mode'] == 'h2v2' for hs, vs in ALL_EIGHT for s in cases.REDUCED)


def test_host_images_equal_the_restatement():
    images, done = cases.host_images()
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    for c in cases.CASES:
        for s in cases.SCALES:
            assert np.array_equal(images[(c.name, s)], cases.expected(c, s)), (c.name, s)


def test_host_baseline_streams():
    streams, results, recoded, done = cases.host_baseline()
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    valid = len(cases.baseline_streams())
    by_case = {'{}/{}'.format(c.name, v): c for c, v, _ in cases.golden_files()}
    for k, s in enumerate(streams[:valid]):
        want = cases.flat_coefficients(by_case[s.name])
        for v in cases.SETTINGS + (0,):
            r = results[(k, v)]
            assert r.status == 0 and np.array_equal(r.coef, want), (s.name, v)
        assert results[(k, 0)].rounds == 0 and recoded[k] == 1, s.name          # and the writer's walks give the file's bytes back
    # damaged: the program ended without a finding of the sanitizers (above); a flipped bit may leave a valid stream, but half a stream,
    # a marker out of sequence and a missing marker never do, at any subsequence length
    for k, s in enumerate(streams[valid:], valid):
        if not s.name.split('|')[-1].startswith('flip'):
            assert all(results[(k, v)].status != 0 for v in cases.SETTINGS + (0,)), s.name


def test_host_progressive_files():
    files, results, done = cases.host_progressive()
    assert results is not None and done.returncode == 0, done.stderr.decode()[-2000:]
    valid = len(cases.progressive_files())
    assert valid == 2 * len(sr.WIDE)
    for f, r in zip(files[:valid], results[:valid]):
        assert r.legal and r.levels == dprog.levels(f.script)
        for v in cases.SETTINGS + (0,):
            assert r.status[v] == 0 and np.array_equal(r.coef[v], f.expected), (f.name, v)
    for f, r in zip(files[valid:], results[valid:]):                  # damaged: no finding of the sanitizers; half a first scan is never whole
        scan = f.name.split('|')[-1]
        if scan.startswith('cut') and f.script[int(scan[3:])][3] == 0:
            assert r.legal and all(r.status[v] != 0 for v in cases.SETTINGS + (0,)), f.name


def test_twins_hold_the_same_coefficients():
    """Baseline, restart, optimised and progressive files of one image: the parsers of the restatement read the same coefficients."""
    for c in cases.CASES:
        if len(c.variants) == 1:
            continue
        want = cases.flat_coefficients(c)
        for v, data in cases.golden()[c.name].files.items():
            if v.startswith('prog'):
                flat, status, _ = dprog.decode(data)
                assert status == 0 and np.array_equal(flat, want), (c.name, v)
            else:
                assert np.array_equal(ref.flat_coefficients(rref.parse(data)['coefs']), want), (c.name, v)
