"""The lossless transforms on the host (no GPU): the rule derived against a float64 inverse DCT, the algebra of the
operations byte for byte on the restatement's files (tests/jpegxform_ref.py), the output files against Pillow - which opens every one
at the swapped size and factors with transposed tables -, the sequential form of csrc/jpegxform.h in a sanitized stand-alone program
against the restatement on every job, lossless_size and every refusal of the Python layer.  Everything but the derivation is exact."""
import io

import numpy as np
import pytest

import jpegxform_cases as cases
import jpegxform_ref as xr
from neural_imaging_amd import _lib, ops
from neural_imaging_amd.compression import jpeg_helpers as jh

ALLOW = dict(allow_restart=True, allow_progressive=True, allow_grey=True, allow_sampling=True)


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('op', xr.OPS)
def test_the_rule_is_the_geometric_operation_on_the_samples(op):
    """Per component plane: the float64 inverse DCT of the transformed, dequantised coefficients with the transformed table is the
    operation on the float64 inverse DCT of the source plane - the rule without libjpeg's rounding."""
    sources, _ = cases.golden()
    for name in ('p422_24x40_prog', 'p420_17x9', 'grey_33x50_rst3', 'w410_16x32'):
        p = xr.parse(sources[name])
        qt = xr.tables(p['qtables'], op)
        for k, comp in enumerate(p['coefs']):
            got = xr.float_plane(xr.component(comp, op), qt[k])
            want = xr.pixels(xr.float_plane(comp, p['qtables'][k]), op)
            assert got.shape == want.shape and np.abs(got - want).max() <= 1e-9, (name, k)


def test_negation_wraps_and_spares_the_dc():
    comp = np.full((1, 1, 64), -32768, np.int16)
    for op in xr.OPS:
        out = xr.component(comp, op)
        assert out[0, 0, 0] == -32768 and (out == -32768).all()                 # -(-32768) stays
    comp = np.arange(1, 65, dtype=np.int16).reshape(1, 1, 64)
    assert xr.component(comp, 'rot180')[0, 0, 0] == 1 and (xr.component(comp, 'hflip') != comp).sum() == 32
    assert sorted(np.abs(xr.component(comp, 'transverse')).reshape(-1).tolist()) == list(range(1, 65))


# ---- the algebra, byte for byte on the restatement's files --------------------------------------------------------------------------------
ALIGNED = ('p444_8x8', 'p420_16x16', 'grey_8x40', 'w410_16x32')                # every operation is perfect on these


@pytest.mark.parametrize('name', ALIGNED)
def test_algebra(name):
    data = cases.golden()[0][name]
    plain = xr.transcode(data)
    once = {op: xr.transcode(data, op) for op in xr.OPS}
    assert once['none'] == plain
    for op in xr.OPS:                                                           # an operation and its inverse
        assert xr.transcode(once[op], xr.INVERSE[op]) == plain, op
    turned = data
    for _ in range(4):
        turned = xr.transcode(turned, 'rot90')
    assert turned == plain
    for op, steps in xr.STEPS.items():                                          # the composition table
        made = data
        for step in steps:
            made = xr.transcode(made, step)
        assert (made if steps else plain) == once[op], op
    p = xr.parse(data)
    assert xr.transcode(data, 'none', crop=(0, 0, p['w'], p['h'])) == plain      # a crop of the whole image


def test_trim_and_crop_commute_with_the_plain_file():
    data = cases.golden()[0]['p444_33x50_opt']
    trimmed = xr.transcode(data, 'rot180', edge='trim')
    assert xr.transcode(trimmed, 'rot180') == xr.transcode(data, 'none', crop=(0, 0, 48, 32))
    assert xr.transcode(data, 'hflip', crop=(8, 8, 16, 9)) == xr.transcode(xr.transcode(data, 'none', crop=(8, 8, 16, 9)), 'hflip')


# ---- against Pillow -----------------------------------------------------------------------------------------------------------------------
def test_golden_is_the_restatement_and_pillow_opens_every_file():
    Image = pytest.importorskip('PIL.Image')
    sources, made = cases.golden()
    parsed = {s.name: xr.parse(sources[s.name]) for s in cases.SOURCES}
    for k, case in enumerate(cases.FILE_CASES):
        m, want, s = made[case.name], cases.expected_size(case), case.source
        if want is None:
            assert m is None
            with pytest.raises(ValueError):
                xr.transcode(sources[s.name], case.op, case.crop, case.edge)
            continue
        if k % 7 == 0 or s.h * s.w <= 256:                                     # the golden file is up to date
            assert xr.transcode(sources[s.name], case.op, case.crop, case.edge) == m.data, case.name
        im = Image.open(io.BytesIO(m.data))
        grey = s.sampling == 'grey'
        assert im.size == m.size == (want[1], want[0]) and im.mode == ('L' if grey else 'RGB'), case.name
        assert [tuple(l) for l in im.layer] == m.layer and im.layer[0][1:3] == ((1, 1) if grey else want[2:]), case.name
        qt = xr.tables(parsed[s.name]['qtables'], case.op)
        assert [list(im.quantization[l[3]]) for l in im.layer] == qt.tolist(), case.name
        px = np.asarray(im)
        assert cases.crc(px) == m.crc and (m.pixels is None or np.array_equal(px, m.pixels)), case.name


def test_vflip_equals_the_flipped_decode_where_nothing_interpolates_vertically():
    """The one pixel identity that holds in general (libjpeg's column pass is odd-symmetric in a negated row, its row pass is not)."""
    Image = pytest.importorskip('PIL.Image')
    sources, made = cases.golden()
    seen = 0
    for case in cases.FILE_CASES:
        s, want = case.source, cases.expected_size(case)
        if case.op != 'vflip' or case.crop is not None or want is None or want[0] != s.h or want[3] > 1:
            continue
        flipped = np.asarray(Image.open(io.BytesIO(sources[s.name])))[::-1]
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(made[case.name].data))), flipped), case.name
        seen += 1
    assert seen >= 4


# ---- the header's sequential form, sanitized ----------------------------------------------------------------------------------------------
def test_host_program_equals_the_restatement_on_every_job():
    results, done = cases.host_jobs()
    assert done.returncode == 0 and not done.stderr, done.stderr.decode(errors='replace')[-2000:]
    refused = 0
    for job in cases.JOBS:
        want, got = cases.job_expected(job), results[job.name]
        if want is None:
            assert got is None, job.name
            refused += 1
            continue
        assert got[0] == cases.job_size(job), job.name
        assert np.array_equal(got[1], want), job.name
    assert 0 < refused < len(cases.JOBS) // 4                                   # 17 x 9 and the narrow strips trim to nothing


QUERIES = [  # (query, reason, what the Python layer's message says)
    (cases.Query(32, 48, 2, 2, 8, None, 'perfect'), 'op', None),
    (cases.Query(32, 48, 2, 2, -1, None, 'perfect'), 'op', None),
    (cases.Query(32, 48, 3, 1, 'none', None, 'perfect'), 'geometry', 'unsupported sampling factors 3x1'),
    (cases.Query(32, 48, 4, 4, 'none', None, 'perfect'), 'geometry', 'unsupported sampling factors 4x4'),
    (cases.Query(0, 48, 1, 1, 'none', None, 'perfect'), 'geometry', 'an image of 0 x 48'),
    (cases.Query(32, 48, 2, 2, 'none', (8, 0, 16, 16), 'perfect'), 'crop align', r'x=8 is not a multiple of the iMCU \(16 .*below is 0'),
    (cases.Query(32, 48, 2, 1, 'none', (16, 12, 16, 16), 'trim'), 'crop align', r'y=12 is not a multiple of the iMCU \(8 .*below is 8'),
    (cases.Query(32, 48, 0, 0, 'none', (8, 8, 16, 16), 'perfect'), 'ok', None),                     # grey-scale: 8 whatever
    (cases.Query(32, 48, 2, 2, 'none', (16, 16, 33, 16), 'perfect'), 'crop outside', 'does not lie inside the 48 x 32 image'),
    (cases.Query(32, 48, 2, 2, 'none', (0, 0, 0, 16), 'perfect'), 'crop outside', 'does not lie inside'),
    (cases.Query(32, 48, 2, 2, 'none', (-16, 0, 16, 16), 'perfect'), 'crop outside', 'does not lie inside'),
    (cases.Query(33, 50, 2, 2, 'hflip', None, 'perfect'), 'partial width', r'hflip: the width 50 is not a multiple of the iMCU \(16\)'),
    (cases.Query(33, 50, 2, 2, 'rot270', None, 'perfect'), 'partial width', 'rot270: the width 50'),
    (cases.Query(33, 50, 2, 2, 'vflip', None, 'perfect'), 'partial height', r'vflip: the height 33 is not a multiple of the iMCU \(16\)'),
    (cases.Query(33, 48, 2, 2, 'rot90', None, 'perfect'), 'partial height', 'rot90: the height 33'),
    (cases.Query(32, 50, 2, 2, 'rot180', None, 'perfect'), 'partial width', 'rot180: the width 50'),
    (cases.Query(33, 48, 2, 2, 'transverse', None, 'perfect'), 'partial height', 'transverse: the height 33'),
    (cases.Query(33, 50, 2, 2, 'transpose', None, 'perfect'), 'ok', None),
    (cases.Query(33, 50, 2, 2, 'none', None, 'perfect'), 'ok', None),
    (cases.Query(33, 50, 2, 2, 'rot180', None, 'trim'), 'ok', None),
    (cases.Query(17, 9, 2, 2, 'hflip', None, 'trim'), 'empty', 'nothing is left of the width 9'),
    (cases.Query(17, 9, 1, 1, 'transverse', (8, 0, 1, 7), 'trim'), 'empty', 'nothing is left of the width 1'),
    (cases.Query(33, 50, 1, 1, 'vflip', (0, 32, 50, 1), 'trim'), 'empty', 'nothing is left of the height 1'),
]


def test_refusals_of_the_header_and_of_the_python_layer_agree():
    got, done = cases.host_geometry([q for q, _, _ in QUERIES])
    assert done.returncode == 0 and not done.stderr, done.stderr.decode(errors='replace')[-2000:]
    for (q, reason, message), (named, geo) in zip(QUERIES, got):
        assert named == reason, q
        if isinstance(q.op, int):
            continue
        if reason == 'ok':
            want = xr.size(q.h, q.w, q.hs, q.vs, q.op, q.crop, q.edge)
            assert jh.lossless_size(q.h, q.w, q.hs, q.vs, q.op, q.crop, q.edge) == want
            assert geo[:2] == want[:2] and geo[2:4] == ((1, 1) if (q.hs, q.vs) == xr.GREY else want[2:])
        else:
            with pytest.raises(ValueError, match=message):
                jh.lossless_size(q.h, q.w, q.hs, q.vs, q.op, q.crop, q.edge)
            if reason != 'geometry':
                with pytest.raises(ValueError):
                    xr.size(q.h, q.w, q.hs, q.vs, q.op, q.crop, q.edge)
    for op, edge in (('rot', 'perfect'), (None, 'perfect'), (5, 'perfect'), ('hflip', 'cut'), ('hflip', None)):
        with pytest.raises(ValueError, match='lossless: one of none, hflip|edge: .perfect'):
            jh.lossless_size(32, 48, 2, 2, op, None, edge)
    for crop in ((0, 0, 16), (0, 0, 16.5, 16), 'abcd', 5):
        with pytest.raises(ValueError, match='crop: '):
            jh.lossless_size(32, 48, 2, 2, 'none', crop)


def test_lossless_size_equals_the_restatement_on_every_job():
    for job in cases.JOBS:
        for edge in ('trim', 'perfect'):
            args = (job.h, job.w) + cases.factors(job.sampling) + (job.op, job.crop, edge)
            try:
                want = xr.size(*args)
            except ValueError:
                with pytest.raises(ValueError):
                    jh.lossless_size(*args)
                continue
            assert jh.lossless_size(*args) == ops.jpeg_lossless_geometry(*args) == want, (job.name, edge)


def test_abi_and_names():
    assert ops.JPEG_LOSSLESS_OPS == xr.OPS and _lib.ABI_VERSION == 8
    for name in ('nimg_jpeg_lossless', 'nimg_jpeg_lossless_geometry'):
        assert name in _lib.PROTOTYPES and hasattr(_lib.load(), name)
    assert len(_lib.PROTOTYPES['nimg_jpeg_lossless'][1]) == 19 and len(_lib.PROTOTYPES['nimg_jpeg_lossless_geometry'][1]) == 15


# ---- transcode_batch refuses on the host ------------------------------------------------------------------------------------------------------
def test_transcode_batch_refuses_before_anything_goes_to_a_device(monkeypatch):
    """Every refusal is a ValueError of the host checks: the decode that would follow them is made to fail the test."""
    sources, _ = cases.golden()

    def reached(*a, **k):
        raise AssertionError('the files went to the device')
    monkeypatch.setattr(jh, '_decode_groups', reached)
    ragged, aligned, grey, tall = sources['p444_33x50_opt'], sources['p420_64x96'], sources['grey_33x50_rst3'], sources['p422_24x40_prog']
    with pytest.raises(ValueError, match=r'file 1 \(50 x 33, width x height\): lossless hflip: the width 50 is not a multiple of the iMCU \(8\)'):
        jh.transcode_batch([aligned, ragged], lossless='hflip', **ALLOW)
    with pytest.raises(ValueError, match=r'file 0 .*lossless vflip: the height 33'):
        jh.transcode_batch([grey], lossless=['vflip'], **ALLOW)
    with pytest.raises(ValueError, match='lossless: one operation for every file or one per file needed, got 1 for 2 files'):
        jh.transcode_batch([aligned, ragged], lossless=['hflip'], **ALLOW)
    with pytest.raises(ValueError, match="lossless: one of none, hflip, .* got 'rot45'"):
        jh.transcode_batch([aligned], lossless='rot45')
    with pytest.raises(ValueError, match="edge: 'perfect'"):
        jh.transcode_batch([aligned], lossless='hflip', edge='keep')
    with pytest.raises(ValueError, match=r'file 0 .*crop: x=8 is not a multiple of the iMCU \(16 .*below is 0'):
        jh.transcode_batch([aligned], crop=(8, 0, 16, 16))
    with pytest.raises(ValueError, match='file 1 .*does not lie inside the 50 x 33 image'):
        jh.transcode_batch([aligned, ragged], crop=(0, 0, 64, 32))
    with pytest.raises(ValueError, match='file 0 .*nothing is left of the width 9'):
        jh.transcode_batch([sources['p420_17x9']], lossless='rot180', edge='trim')
    with pytest.raises(ValueError, match='progressive=True: progressive files are not written with the sampling factors 1x2'):
        jh.transcode_batch([tall], lossless='transpose', progressive=True, allow_progressive=True)       # 4:2:2 comes out as 4:4:0
    with pytest.raises(ValueError, match='grey-scale .one-component. images: progressive=True'):
        jh.transcode_batch([grey], lossless='transpose', progressive=True, **ALLOW)
    with pytest.raises(ValueError, match='unsupported sampling factors'):                               # reading stays behind its keyword
        jh.transcode_batch([sources['w440_24x40']], lossless='transpose')
    with pytest.raises(AssertionError, match='went to the device'):                                     # what is not refused goes on
        jh.transcode_batch([sources['w440_24x40']], lossless='transpose', progressive=True, allow_sampling=True)      # 4:4:0 -> 4:2:2
