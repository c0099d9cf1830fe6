"""The baseline JPEG codec on the host (no GPU): the plain numpy restatement of the format (tests/jpeg_ref.py) against Pillow /
libjpeg and against the committed golden files, what the case list reaches, and the host half of the product
(compression.jpeg_helpers: header, libjpeg's tables, JPEGMarkerStats)."""
import io

import numpy as np
import pytest

import jpeg_cases as cases
import jpeg_ref as ref
from neural_imaging_amd.compression import jpeg_helpers as jh


def _pillow(img, quality, subsampling):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format='JPEG', quality=quality, subsampling=cases.SUBSAMPLINGS.index(subsampling))
    return buf.getvalue(), np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert('RGB'))


def test_restatement_equals_pillow():
    """Whole files and decoded images, every case; the parser finds the encoder's coefficients in Pillow's file."""
    pytest.importorskip('PIL')
    for case in cases.CASES:
        r = cases.reference(case)
        for i, img in enumerate(cases.build(case)):
            data, rgb = _pillow(img, case.quality, case.subsampling)
            assert r.files[i] == data, case.name
            assert np.array_equal(r.decoded[i], rgb), case.name
            parsed = ref.parse(data)
            assert (parsed['h'], parsed['w'], parsed['ecd_offset']) == (case.h, case.w, ref.HEADER_BYTES)
            for k, c in enumerate(r.coefs[i]):
                assert np.array_equal(parsed['coefs'][k][:c.shape[0], :c.shape[1]], c), (case.name, k)


@pytest.mark.parametrize('size', [(1, 1), (2, 2), (3, 5), (5, 3), (9, 4), (7, 6)])
def test_restatement_equals_pillow_on_tiny_images(size):
    """Up to two chroma columns libjpeg replicates instead of filtering; one block, mostly padding."""
    pytest.importorskip('PIL')
    img = np.random.default_rng(size[0] * 16 + size[1]).integers(0, 256, size + (3,), dtype=np.uint8)
    for subsampling in cases.SUBSAMPLINGS:
        data, rgb = _pillow(img, 90, subsampling)
        mine, decoded = ref.compress(img, 90, subsampling)
        assert mine == data and np.array_equal(decoded, rgb), (size, subsampling)


def test_restatement_equals_golden():
    golden = cases.golden()
    assert sorted(golden) == sorted(c.name for c in cases.GOLDEN_CASES)
    for case in cases.GOLDEN_CASES:
        x, files, rgb = golden[case.name]
        r = cases.reference(case)
        assert np.array_equal(x, cases.build(case)), case.name
        assert files == r.files, case.name
        assert np.array_equal(rgb, r.decoded), case.name


def test_case_list_reaches_every_path():
    """A case list that no longer reaches a path of the coder must say so."""
    total = {}
    for case in cases.CASES:
        for key, v in cases.reference(case).stats.items():
            total[key] = total.get(key, 0) + int(v)
    for key in ('stuffed', 'zrl', 'ac10', 'dc11', 'dummy_right', 'dummy_bottom', 'pad_some', 'pad_none'):
        assert total[key] > 0, key
    assert {c.quality for c in cases.CASES} == set(cases.QUALITIES)
    assert {c.subsampling for c in cases.CASES} == set(cases.SUBSAMPLINGS)
    # the inputs named for a path reach it
    assert cases.reference(cases.by_name('noise_16x24_q100_444')).stats['stuffed'] > 0
    assert cases.reference(cases.by_name('checker_16x16_q100_444')).stats['ac10'] > 0
    assert cases.reference(cases.by_name('half_16x16_q100_444')).stats['dc11'] > 0
    assert cases.reference(cases.by_name('cosine_16x24_q75_444')).stats['zrl'] > 0
    constant = cases.reference(cases.by_name('constant_16x16_q75_444'))
    assert all(not c[..., 1:].any() for c in constant.coefs[0]) and np.ptp(constant.coefs[0][0][..., 0]) == 0


def test_libjpeg_tables():
    """The product's libjpeg_qtable is the restatement's; with Pillow, both are what libjpeg writes at every quality."""
    for q in range(1, 101):
        for ch in (0, 1):
            assert np.array_equal(jh.libjpeg_qtable(q, ch).ravel(), ref.qtable(q, ch)), (q, ch)
    # the differentiable codec's jpeg_qtable scales by the real 5000 / q (the reference's Python): one more where libjpeg's integer
    # quotient loses a fraction, identical wherever q divides 5000 and from 50 on
    differ = [q for q in range(1, 101) if not np.array_equal(jh.libjpeg_qtable(q, 0), jh.jpeg_qtable(q, 0))]
    assert 30 in differ and all(q < 50 and 5000 % q for q in differ)
    pytest.importorskip('PIL')
    from PIL import Image
    for q in range(1, 101):
        buf = io.BytesIO()
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(buf, format='JPEG', quality=q)
        parsed = ref.parse(buf.getvalue())
        for ch in (0, 1):
            assert np.array_equal(parsed['qtables'][ch], ref.qtable(q, ch)), (q, ch)


def test_header_equals_golden():
    for case in cases.GOLDEN_CASES:
        for data in cases.golden()[case.name][1]:
            head = jh.jpeg_header(case.h, case.w, case.quality, case.subsampling)
            assert len(head) == jh.JPEG_HEADER_BYTES == 623 and head == data[:623], case.name
    with pytest.raises(ValueError):
        jh.jpeg_header(8, 8, 75, '4:1:1')


def test_marker_stats_on_golden_files(tmp_path):
    for name in ('mixed_40x56_q1_420', 'noise+smooth+constant+checker_16x24_q75_422'):
        case = cases.by_name(name)
        for data in cases.golden()[name][1]:
            s = jh.JPEGMarkerStats(data)
            assert list(s.blocks) == ['SOI', 'APP:0/0', 'DQT:0', 'DQT:1', 'DCT', 'DHT:0', 'DHT:16', 'DHT:1', 'DHT:17', 'SOS', 'ECD', 'EOI']
            assert [s.blocks[k] for k in s.blocks] == [0, 2, 20, 89, 158, 177, 210, 393, 426, 609, 623, len(data)]
            assert s.shape == (case.h, case.w, 3)
            assert s.get_bytes() == len(data) and s.get_effective_bytes() == len(data) - 177
            assert s.get_bpp() == 8 * len(data) / case.h / case.w
            assert s.get_effective_bpp() == 8 * (len(data) - 177) / case.h / case.w
            for ch in (0, 1):
                assert np.array_equal(s._quantization_tables[ch].ravel(), ref.qtable(case.quality, ch))
    path = tmp_path / 'a.jpg'
    path.write_bytes(data)
    assert jh.JPEGMarkerStats(str(path)).blocks == s.blocks


def test_marker_stats_errors():
    data = cases.golden()['smooth_8x8_q50_444'][1][0]
    with pytest.raises(ValueError):
        jh.JPEGMarkerStats(bytearray(data))
    for cut in (3, 100, 400, 622, len(data) - 1):                       # inside a length, a table, the header's end, EOI
        with pytest.raises(IOError):
            jh.JPEGMarkerStats(data[:cut])
    progressive = data[:158] + b'\xff\xc2' + data[160:]
    with pytest.raises(IOError, match='Progressive'):
        jh.JPEGMarkerStats(progressive)


def test_byte_conversion_quirk():
    """(255 * (k / 255)) truncated in float32 - the reference's conversion: the restatement's to_bytes is numpy's arithmetic on all
    256 byte values, with and without the division, truncates, and clamps where numpy's cast would wrap."""
    k = np.arange(256, dtype=np.uint8)
    expect = (255 * (k.astype(np.float32) / 255)).astype(np.uint8)
    assert np.array_equal(ref.to_bytes(k.astype(np.float32)), expect)                     # maximum > 1: divided first
    unit = k.astype(np.float32) / np.float32(255)
    assert np.array_equal(ref.to_bytes(unit), expect)                                     # already in [0, 1]
    assert np.array_equal(ref.to_bytes(np.array([-0.5, 0.0, 0.9999, 1.0], np.float32)), [0, 0, 254, 255])
    assert np.array_equal(ref.to_bytes(np.array([-3.0, 254.9, 300.0], np.float32)), [0, 254, 255])
    assert np.array_equal(ref.to_bytes(k), k)                                             # bytes are taken as they are
