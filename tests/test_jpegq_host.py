"""JPEG files with caller-given quantisation tables, the parts that need no GPU: the numpy restatement
(tests/jpegq_ref.py) against Pillow's golden files, jpeg_helpers.jpeg_header(qtables=) and check_qtables, the refusals that come
before any device is touched, and the float-to-table rule.  Everything is exact."""
import numpy as np
import pytest

import jpegq_cases as cases
import jpegq_ref as qref
from neural_imaging_amd.compression import jpeg_helpers as jh

RULE = cases.RULE


@pytest.mark.parametrize('case', cases.CASES, ids=cases.IDS)
def test_restatement_equals_pillow(case):
    g = cases.golden()[case.name]
    r = cases.restated(case)
    assert r.file == g.file and np.array_equal(r.decoded, g.rgb)
    t = len(cases.tables(case.kind))
    assert g.file.index(b'\xff\xc4') == qref.DHT_OFFSET[t] and g.file.index(b'\xff\xda') + 14 == qref.HEADER_BYTES[t]
    if g.optimized is not None:
        assert cases.restated(case, True).file == g.optimized
    assert (g.optimized is not None) == (case in cases.OPTIMIZED)


def test_golden_equals_a_fresh_pillow_run():
    pytest.importorskip('PIL')
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import make_jpegq_golden as make
    g = cases.golden()
    for case in cases.CASES:
        data, rgb = make.pillow(cases.image(case), cases.tables(case.kind), case.subsampling)
        assert data == g[case.name].file and np.array_equal(rgb, g[case.name].rgb), case.name
    for case in cases.OPTIMIZED:
        assert make.pillow(cases.image(case), cases.tables(case.kind), case.subsampling, optimize=True)[0] == g[case.name].optimized


@pytest.mark.parametrize('case', cases.CASES, ids=cases.IDS)
def test_header_with_tables(case):
    g = cases.golden()[case.name]
    t = cases.tables(case.kind)
    head = jh.jpeg_header(case.h, case.w, None, case.subsampling, qtables=t)
    assert len(head) == {2: 623, 3: 692}[len(t)] == qref.HEADER_BYTES[len(t)] and g.file.startswith(head)
    assert head == jh.jpeg_header(case.h, case.w, None, case.subsampling, qtables=t.reshape(-1, 8, 8).tolist())
    assert jh._header_bytes(t) == (qref.HEADER_BYTES[len(t)], qref.DHT_OFFSET[len(t)])
    hd = jh.parse_header(g.file)
    assert np.array_equal(hd.qtables, qref.per_component(t))
    if g.optimized is not None:                                     # huffman= combines with it: the optimised file's header
        o = jh.parse_header(g.optimized)
        import jpegopt_ref as oref
        huffman = np.stack([oref.table_of(c, s) for c, s in o.huffman[:4]])
        head = jh.jpeg_header(case.h, case.w, None, case.subsampling, huffman=huffman, qtables=t)
        assert g.optimized.startswith(head) and len(head) == o.ecd_offset


def test_header_with_a_quality_is_unchanged():
    for q in (1, 30, 49, 75, 100):
        pair = [jh.libjpeg_qtable(q, 0), jh.libjpeg_qtable(q, 1)]
        assert jh.jpeg_header(13, 21, q, '4:2:0') == jh.jpeg_header(13, 21, None, '4:2:0', qtables=pair)
    assert jh.jpeg_header(8, 8, 0) == jh.jpeg_header(8, 8, 1) and jh.jpeg_header(8, 8, 250) == jh.jpeg_header(8, 8, 100)


def test_check_qtables():
    good = np.arange(1, 129).reshape(2, 64)
    for form in (good, good.reshape(2, 8, 8), good.tolist(), good.astype(np.float32), good.astype(np.uint8)):
        out = jh.check_qtables(form)
        assert out.dtype == np.uint16 and out.shape == (2, 64) and np.array_equal(out, good)
    assert jh.check_qtables(np.full((3, 64), 255)).shape == (3, 64)

    def refused(t, match):
        with pytest.raises(ValueError, match=match):
            jh.check_qtables(t)

    bad = good.copy()
    bad[1, 10] = 0
    refused(bad, r'entry 10 \(row 1, column 2\) of table 1 is 0\.0')
    bad[1, 10] = 256
    refused(bad, r'entry 10 \(row 1, column 2\) of table 1 is 256\.0')
    bad = good.astype(np.float64)
    bad[0, 63] = 1.5
    refused(bad, r'entry 63 \(row 7, column 7\) of table 0 is 1\.5')
    bad[0, 63] = np.nan
    refused(bad, r'entry 63 .* of table 0 is nan')
    bad[0, 63] = -4
    refused(bad, r'of table 0 is -4\.0')
    refused(good[:1], r'2 tables \(luma, chroma\) or 3 \(Y, Cb, Cr\) needed, got 1')
    refused(np.ones((4, 64)), r'needed, got 4')
    refused(np.ones((2, 63)), r'shape \(T, 64\) or \(T, 8, 8\) needed, got \(2, 63\)')
    refused(np.ones((2, 8, 4)), r'shape')
    refused(np.ones(128), r'shape')
    refused(np.ones((1, 2, 8, 8)), r'shape')
    refused('tables', r'numbers needed')
    refused(None, r'numbers needed')


def test_quality_and_qtables_exclude_each_other(monkeypatch):
    """Refused on the host: the upload is never reached."""
    def no_device(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(jh, '_device_batch', no_device)
    monkeypatch.setattr(jh.ops, 'jpeg_transform', no_device)
    monkeypatch.setattr(jh.ops, 'jpeg_transform_tables', no_device)
    x = np.zeros((1, 8, 8, 3), np.uint8)
    t = np.ones((2, 64))
    for call in (lambda q, t: jh.encode_batch(x, q, qtables=t), lambda q, t: jh.compress_batch(x, q, qtables=t),
                 lambda q, t: jh.compress_batch(x[0], q, optimize=True, qtables=t), lambda q, t: jh.device_codec(x, q, qtables=t),
                 lambda q, t: jh.jpeg_header(8, 8, q, qtables=t)):
        with pytest.raises(ValueError, match='both were given'):
            call(75, t)
        with pytest.raises(ValueError, match='neither were given'):
            call(None, None)
    with pytest.raises(ValueError, match='table 0'):
        jh.encode_batch(x, None, qtables=np.zeros((2, 64)))
    with pytest.raises(ValueError, match='table 1'):
        jh.rate_distortion_tables(x, [np.ones((2, 64)), [[1] * 64, [1] * 63 + [300]]])
    with pytest.raises(ValueError, match='table sets'):
        jh.rate_distortion_tables(x, np.ones((2, 64)))


def test_float_rule():
    values = np.array([v for v, _, _ in RULE], np.float32)
    for n_tabs in (2, 3):
        for k, (v, entry, status) in enumerate(RULE):
            t = np.full((1, n_tabs, 64), 7.0, np.float32)
            t[0, n_tabs - 1, k] = v
            q, st = qref.tables_from_float(t)
            assert q.shape == (1, 3, 64) and q.dtype == np.uint16 and st.tolist() == [status], v
            assert q[0, 2, k] == entry and (np.delete(q.reshape(-1), [128 + k] + ([64 + k] if n_tabs == 2 else [])) == 7).all(), v
            assert np.array_equal(q[0, 1], q[0, 2]) == (n_tabs == 2 or entry == 7)
            assert qref.moved(t).reshape(-1).nonzero()[0].tolist() == ([(n_tabs - 1) * 64 + k] if status else [])
    t = np.full((2, 2, 64), 9.0, np.float32)
    t[1, 0, :len(values)] = values                                      # the bits of a set are OR-ed, the other set stays clean
    q, st = qref.tables_from_float(t)
    assert st.tolist() == [0, 7] and q[1, 0, :len(values)].tolist() == [e for _, e, _ in RULE] and (q[0] == 9).all()
