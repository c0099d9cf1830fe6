"""JPEG files with any quantisation tables on the GPU (csrc/jpegc_tables.hip through ops.jpeg_transform_tables /
jpeg_tables_from_float, the qtables= paths of compression.jpeg_helpers, rate_distortion_tables, transcode_batch and
JPEG.file_tables / process_files): whole files and decoded images against Pillow's golden files, the quality path, the single-item
call and the numpy restatement (tests/jpegq_ref.py) - everything exact, nothing has a tolerance."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

import jpeg_cases
import jpeg_ref
import jpegd_cases
import jpegopt_cases
import jpegq_cases as cases
import jpegq_ref as qref
import ratedist_cases
from neural_imaging_amd import ops
from neural_imaging_amd.compression import jpeg_helpers as jh

pytestmark = pytest.mark.gpu

GUARD = 256


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()
    return torch.device('cuda', 0)


def _guarded(shape, dtype, fill, dev):
    """(the whole buffer as bytes, a view of `shape` with GUARD canary bytes in front of it and behind it)."""
    size = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    whole = torch.full((size + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
    return whole, whole[GUARD:GUARD + size].view(dtype).view(shape)


def _intact(whole, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _device_sets(sets, items, dev):
    """(K, T, 64) -> (K * items, 3, 64) int16 device tensor, set-major."""
    t = np.stack([qref.per_component(s) for s in sets]).astype(np.uint16)
    return torch.from_numpy(np.repeat(t, items, axis=0).view(np.int16)).to(dev)


def _libjpeg_pair(q):
    return np.stack([jh.libjpeg_qtable(q, 0).ravel(), jh.libjpeg_qtable(q, 1).ravel()])


@contextlib.contextmanager
def _quiet():
    """(images this small have no MS-SSIM: helpers.metrics says so, once per process, in a warning)"""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        yield


def _sources(n, h, w):
    """uint8 (n, h, w, 3): noise, smooth, mixed, checker in turn."""
    return np.stack([jpeg_cases._image(ratedist_cases.CONTENTS[i % 4], h, w, 31 + i) for i in range(n)])


# ---- 1. every golden case: libjpeg's files and images ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', cases.CASES, ids=cases.IDS)
def test_golden_case(dev, case):
    g, t, x = cases.golden()[case.name], cases.tables(case.kind), cases.image(case)[None]
    files = jh.encode_batch(x, None, case.subsampling, qtables=t)
    assert files == [g.file], 'not the file libjpeg writes with these tables'
    want = g.rgb[None].astype(np.float32) / np.float32(255)
    head, dht = qref.HEADER_BYTES[len(t)], qref.DHT_OFFSET[len(t)]
    assert g.file.index(b'\xff\xc4') == dht and jh.parse_header(g.file).ecd_offset == head
    for batch in (x, x.astype(np.float32) / np.float32(255)):
        y, sizes = jh.compress_batch(batch, None, subsampling=case.subsampling, qtables=t)
        assert y.dtype == np.float32 and np.array_equal(_bits(y), _bits(want)) and sizes == [len(g.file)]
        assert jh.compress_batch(batch, None, True, case.subsampling, qtables=t)[1] == [len(g.file) - dht]
    y1, size1 = jh.compress_batch(x[0], None, subsampling=case.subsampling, qtables=t.reshape(-1, 8, 8))
    assert isinstance(size1, int) and size1 == len(g.file) and np.array_equal(y1, g.rgb / 255)
    assert np.array_equal(jh.decode_batch(files), g.rgb[None])
    if g.optimized is not None:
        assert jh.encode_batch(x, None, case.subsampling, optimize=True, qtables=t) == [g.optimized]
        y, sizes = jh.compress_batch(x, None, subsampling=case.subsampling, optimize=True, qtables=t)
        assert np.array_equal(_bits(y), _bits(want)) and sizes == [len(g.optimized)]
        assert jh.compress_batch(x, None, True, case.subsampling, optimize=True, qtables=t)[1] == [len(g.optimized) - dht]
        assert np.array_equal(jh.decode_batch(g.optimized), g.rgb[None])


def test_two_and_three_tables_have_one_effective_size(dev):
    x = _sources(2, 17, 33)
    pair = cases.tables('random')
    triple = pair[[0, 1, 1]]
    a, b = jh.encode_batch(x, None, '4:2:0', qtables=pair), jh.encode_batch(x, None, '4:2:0', qtables=triple)
    assert [len(f) + 69 for f in a] == [len(f) for f in b] and [f[623:] for f in a] == [f[692:] for f in b]
    for optimize in (False, True):
        ya, sa = jh.compress_batch(x, None, True, '4:2:0', optimize=optimize, qtables=pair)
        yb, sb = jh.compress_batch(x, None, True, '4:2:0', optimize=optimize, qtables=triple)
        assert sa == sb and np.array_equal(_bits(ya), _bits(yb))
        whole = jh.compress_batch(x, None, False, '4:2:0', optimize=optimize, qtables=triple)[1]
        assert whole == [s + 246 for s in sb] == [s + 177 + 69 for s in sa]


# ---- 2. identity with the quality path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('subsampling', jpeg_cases.SUBSAMPLINGS)
def test_libjpeg_tables_give_the_quality_path(dev, subsampling):
    hs, vs = ops.jpeg_subsampling(subsampling)
    x = _sources(3, 24, 40)
    xd = torch.from_numpy(x).to(dev)
    for q in (1, 5, 30, 49, 50, 75, 95, 100):
        pair = [jh.libjpeg_qtable(q, 0), jh.libjpeg_qtable(q, 1)]
        assert jh.encode_batch(x, None, subsampling, qtables=pair) == jh.encode_batch(x, q, subsampling), q
        coef, err = ops.jpeg_transform_tables(xd, _device_sets([_libjpeg_pair(q)], 3, dev), hs, vs)
        assert torch.equal(coef, ops.jpeg_transform(xd, q, hs, vs)) and int(err.item()) == 0, q
    xf = x.astype(np.float32) / np.float32(255)
    y, sizes = jh.compress_batch(xf, None, subsampling=subsampling, optimize=True, qtables=_libjpeg_pair(30))
    y0, sizes0 = jh.compress_batch(xf, 30, subsampling=subsampling, optimize=True)
    assert sizes == sizes0 and np.array_equal(_bits(y), _bits(y0))


# ---- 3. items: K table sets over n images in one call ---------------------------------------------------------------------------
ITEM_SETS = ('random', 'three', 'learned', 'max')


@pytest.mark.parametrize('h,w,subsampling', [(24, 40, '4:4:4'), (17, 33, '4:2:2')])
def test_every_item_equals_its_image_alone_with_its_tables(dev, h, w, subsampling):
    hs, vs = ops.jpeg_subsampling(subsampling)
    x = _sources(3, h, w)
    xd = torch.from_numpy(x).to(dev)
    sets = [cases.tables(k) for k in ITEM_SETS]
    qt = _device_sets(sets, 3, dev)
    coef, err = ops.jpeg_transform_tables(xd, qt, hs, vs)
    assert tuple(coef.shape) == (12, ops.jpeg_geometry(h, w, hs, vs)[0], 64) and int(err.item()) == 0
    y = ops.jpeg_reconstruct_tables(coef, h, w, qt, hs, vs)
    data, lengths = ops.jpeg_encode(coef, h, w, hs, vs)
    ends = np.concatenate([[0], np.cumsum(lengths.cpu().numpy().astype(np.int64))])
    blob = data.cpu().numpy()
    for j in range(12):
        k, i = divmod(j, 3)
        alone, e1 = ops.jpeg_transform_tables(xd[i:i + 1].contiguous(), qt[j:j + 1].contiguous(), hs, vs)
        assert torch.equal(coef[j:j + 1], alone) and int(e1.item()) == 0, j
        want_file, want_rgb, want_flat = qref.compress(x[i], sets[k], subsampling)
        assert np.array_equal(coef[j].cpu().numpy().reshape(-1), want_flat), j
        assert blob[ends[j]:ends[j + 1]].tobytes() == want_file[qref.HEADER_BYTES[len(sets[k])]:-2], j
        assert np.array_equal(_bits(y[j].cpu().numpy()), _bits(want_rgb.astype(np.float32) / np.float32(255))), j
    # float input: one above-one flag per call over the sources, whatever the tables
    xf = x.astype(np.float32) / np.float32(255)
    xf[1] = x[1]
    cf, _ = ops.jpeg_transform_tables(torch.from_numpy(xf).to(dev), qt, hs, vs)
    divided = torch.from_numpy(jpeg_ref.to_bytes(xf)).to(dev)
    assert torch.equal(cf, ops.jpeg_transform_tables(divided, qt, hs, vs)[0]) and not torch.equal(cf, coef)


@pytest.mark.parametrize('h,w,subsampling', [(24, 40, '4:4:4'), (17, 33, '4:2:2')])
def test_rate_distortion_tables_equals_the_loop(dev, h, w, subsampling):
    from neural_imaging_amd.helpers import metrics
    x = _sources(3, h, w).astype(np.float32) / np.float32(255)
    for names, effective, optimize in ((('random', 'learned', 'max', 'ones'), True, False), (('three', 'three'), False, True)):
        sets = np.stack([cases.tables(k) for k in names])
        with _quiet():
            out, images = jh.rate_distortion_tables(x, sets, subsampling=subsampling, effective=effective, want_images=True,
                                                    optimize=optimize)
        assert set(out) == {'ssim', 'psnr', 'msssim', 'msssim_db', 'bytes', 'bpp'}
        assert tuple(images.shape) == (len(sets), 3, h, w, 3) and images.is_cuda
        images = images.cpu().numpy()
        for k in range(len(sets)):
            y, sizes = jh.compress_batch(x, None, effective, subsampling, optimize=optimize, qtables=sets[k])
            assert out['bytes'][k].tolist() == sizes, (names[k], effective, optimize)
            assert np.array_equal(_bits(images[k]), _bits(y))
            with _quiet():
                assert np.array_equal(out['ssim'][k], metrics.ssim(x, y)) and np.array_equal(out['psnr'][k], metrics.psnr(x, y))
                assert np.array_equal(out['msssim'][k], metrics.msssim(x, y), equal_nan=True)
        assert out['bytes'].shape == (len(sets), 3) and np.array_equal(out['bpp'], 8 * out['bytes'] / h / w)


def test_rate_distortion_tables_with_libjpeg_tables_equals_rate_distortion(dev, monkeypatch):
    x = ratedist_cases.rd_images(176, 192)[:2]
    qualities = (95, 49, 30)
    sets = np.stack([_libjpeg_pair(q) for q in qualities])
    for subsampling, optimize in (('4:2:0', False), ('4:4:4', True)):
        want = jh.rate_distortion(x, qualities, subsampling=subsampling, optimize=optimize)
        calls = []
        real = ops.jpeg_transform_tables
        monkeypatch.setattr(ops, 'jpeg_transform_tables', lambda *a, **k: calls.append(1) or real(*a, **k))
        got = jh.rate_distortion_tables(x, sets, subsampling=subsampling, optimize=optimize)
        assert len(calls) == 1                                        # K * n items in one transform call
        assert all(np.array_equal(want[key], got[key]) for key in want), (subsampling, optimize)
        hs, vs = ops.jpeg_subsampling(subsampling)
        monkeypatch.setattr(jh, 'RD_WORKSPACE_BUDGET', int(ops._lib.load().nimg_jpeg_workspace_bytes(2, 176, 192, hs, vs)))
        parts = jh.rate_distortion_tables(x, sets.reshape(3, 2, 8, 8), subsampling=subsampling, optimize=optimize)
        assert len(calls) == 1 + len(qualities) and all(np.array_equal(want[key], parts[key]) for key in want)
        monkeypatch.undo()


# ---- 4. tables outside 1..255 on the device --------------------------------------------------------------------------------------
def test_out_of_range_entry_is_clamped_and_flagged(dev):
    """Past check_qtables, straight to the ABI: the kernel divides by the clamped entry and raises the flag; nothing is written
    outside the coefficients, nothing in the tables."""
    from neural_imaging_amd import _lib
    h, w, hs, vs = 17, 33, 2, 2
    x = torch.from_numpy(_sources(3, h, w)).to(dev)
    nb = ops.jpeg_geometry(h, w, hs, vs)[0]
    good = np.repeat(qref.per_component(cases.tables('random'))[None], 3, axis=0).astype(np.uint16)
    good[1, 0, 5], good[2, 2, 63] = 1, 255
    bad = good.copy()
    bad[1, 0, 5], bad[2, 2, 63] = 0, 300                               # a zero in a luma table, 300 in the last item's Cr table
    ws = torch.empty(int(_lib.load().nimg_jpeg_workspace_bytes(3, h, w, hs, vs)), dtype=torch.uint8, device=dev)

    def run(tables):
        qt_all, qt = _guarded((3, 3, 64), torch.int16, 0x6b, dev)
        qt.copy_(torch.from_numpy(tables.view(np.int16)).to(dev))
        coef_all, coef = _guarded((3, nb, 64), torch.int16, 0x5a, dev)
        err = torch.zeros((1,), dtype=torch.int32, device=dev)
        _lib.call('nimg_jpeg_transform_tables', x.data_ptr(), 1, 3, h, w, hs, vs, qt.data_ptr(), 3, coef.data_ptr(), err.data_ptr(),
                  ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert _intact(coef_all, 0x5a) and _intact(qt_all, 0x6b), 'a write outside the coefficients or the tables'
        assert np.array_equal(qt.cpu().numpy().view(np.uint16), tables), 'the tables were written'
        return coef.clone(), int(err.item())

    want, err0 = run(good)
    got, err1 = run(bad)
    assert err0 == 0 and err1 == 1 and torch.equal(got, want)
    assert torch.equal(want, ops.jpeg_transform_tables(x, torch.from_numpy(good.view(np.int16)).to(dev), hs, vs)[0])
    for item, comp, entry, value in ((0, 1, 0, 0), (2, 2, 63, 0xffff), (1, 0, 31, 256)):        # one offender, wherever it sits
        only = good.copy()
        only[item, comp, entry] = value
        assert run(only)[1] == 1, (item, comp, entry)
    with pytest.raises(RuntimeError):
        ops.jpeg_transform_tables(x, torch.from_numpy(good[:, :2].copy().view(np.int16)).to(dev), hs, vs)
    with pytest.raises(RuntimeError):
        ops.jpeg_transform_tables(x, torch.from_numpy(good.astype(np.float32)).to(dev), hs, vs)


# ---- 5. float tables -> file tables -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_tabs', [2, 3])
def test_tables_from_float(dev, n_tabs):
    from neural_imaging_amd import _lib
    RULE = cases.RULE
    named = np.full((3, n_tabs, 64), 7.0, np.float32)
    named[1, n_tabs - 1, :len(RULE)] = [v for v, _, _ in RULE]
    named[2, 0, 3] = 0.5
    rng = np.random.default_rng(20251019 + n_tabs)
    t = np.concatenate([named, rng.uniform(-5, 300, 1000 * n_tabs * 64).astype(np.float32).reshape(1000, n_tabs, 64)])
    t[5] = np.rint(np.clip(t[5], 1, 255))                                # a set the rule leaves alone
    t[6] = np.rint(t[6]) + np.float32(0.5)                              # ties everywhere
    want, want_status = qref.tables_from_float(t)
    assert want_status[:3].tolist() == [0, 7, 1] and want_status[5] == 0 and set(want_status.tolist()) >= {0, 1, 2, 3}
    n = len(t)
    q_all, q = _guarded((n, 3, 64), torch.int16, 0x3c, dev)
    st_all, st = _guarded((n,), torch.int32, 0x3c, dev)
    td = torch.from_numpy(t).to(dev)
    _lib.call('nimg_jpeg_tables_from_float', td.data_ptr(), n, n_tabs, q.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert _intact(q_all, 0x3c) and _intact(st_all, 0x3c)
    assert np.array_equal(q.cpu().numpy().view(np.uint16), want) and np.array_equal(st.cpu().numpy(), want_status)
    q2, st2 = ops.jpeg_tables_from_float(td.view(n, n_tabs, 8, 8))
    assert torch.equal(q2, q) and torch.equal(st2, st) and q2.dtype == torch.int16 and tuple(q2.shape) == (n, 3, 64)
    one = ops.jpeg_tables_from_float(td[1:2].contiguous())
    assert np.array_equal(one[0].cpu().numpy().view(np.uint16), want[1:2]) and one[1].cpu().tolist() == [7]
    with pytest.raises(RuntimeError):
        ops.jpeg_tables_from_float(td[:, :1].contiguous())
    with pytest.raises(RuntimeError):
        ops.jpeg_tables_from_float(td.double())


# ---- 6. transcode -----------------------------------------------------------------------------------------------------------------
def test_transcode_between_plain_and_optimised_golden_files(dev):
    plain, optimised = jpeg_cases.golden(), jpegopt_cases.golden()
    names = [n for n in plain if n in optimised]
    assert len(names) == len(jpeg_cases.GOLDEN_CASES)
    a = [f for n in names for f in plain[n][1]]
    b = [f for n in names for f in optimised[n]]
    assert len(a) == len(b) == 47
    assert jh.transcode_batch(a, optimize=True) == b                    # mixed geometries in one call, results in input order
    assert jh.transcode_batch(b, optimize=False) == a
    assert jh.transcode_batch(a[3]) == [b[3]] and jh.transcode_batch(a[:1], optimize=False) == a[:1]


def test_transcode_of_foreign_files(dev):
    files = [f.data for f in jpegd_cases.foreign_files()]
    names = [f.name for f in jpegd_cases.foreign_files()]
    assert any('qt-high' in n for n in names) and any('qt-reversed' in n for n in names)
    for optimize in (True, False):
        out = jh.transcode_batch(files, optimize=optimize)
        assert len(out) == len(files)
        for name, f, o in zip(names, files, out):
            hf, ho = jh.parse_header(f), jh.parse_header(o)
            assert (hf.h, hf.w, hf.hs, hf.vs) == (ho.h, ho.w, ho.hs, ho.vs) and np.array_equal(hf.qtables, ho.qtables), name
            cf, co = jh.decode_coefficients(f, device_output=True)[0], jh.decode_coefficients(o, device_output=True)[0]
            assert torch.equal(cf, co), name
            assert o[:20] == files[0][:2] + bytes.fromhex('ffe000104a46494600010100000100010000') and o.count(b'\xff\xdb') >= 2
            assert b'\xff\xfe' not in o[:ho.ecd_offset] and o.count(b'\xff\xe0') == 1              # COM and further APPn are dropped
            if not optimize:
                assert ho.ecd_offset == (623 if np.array_equal(hf.qtables[1], hf.qtables[2]) else 692), name
        decoded, again = jh.decode_batch(files), jh.decode_batch(out)
        assert all(np.array_equal(p, q) for p, q in zip(decoded, again))
        assert all(np.array_equal(p, f.rgb) for p, f in zip(again, jpegd_cases.foreign_files()))
        assert jh.transcode_batch(out, optimize=optimize) == out        # a second transcode is the identity
    with pytest.raises(ValueError, match='damaged JPEG data'):
        f = files[names.index('mixed_40x56_420_q75_opt')]
        hd = jh.parse_header(f)
        jh.transcode_batch([files[0], f[:hd.ecd_offset + 40] + f[hd.ecd_end:]])


def test_transcode_with_three_tables(dev):
    x = _sources(2, 17, 33)
    files = jh.encode_batch(x, None, '4:2:2', qtables=cases.tables('three'))
    opt = jh.encode_batch(x, None, '4:2:2', optimize=True, qtables=cases.tables('three'))
    assert jh.transcode_batch(files) == opt and jh.transcode_batch(opt, optimize=False) == files
    assert all(jh.parse_header(f).ecd_offset == 692 for f in files)


# ---- 7. the JPEG model ------------------------------------------------------------------------------------------------------------
def test_model_with_the_differentiable_codecs_tables(dev):
    from neural_imaging_amd.models.jpeg import JPEG
    x = _sources(3, 24, 40).astype(np.float32) / np.float32(255)
    model = JPEG(quality=30, codec='soft', device=dev)
    tables, clamped = model.file_tables()
    soft = np.stack([jh.jpeg_qtable(30, 0).ravel(), jh.jpeg_qtable(30, 1).ravel()])
    assert tables.dtype == np.uint16 and tables.shape == (2, 64) and clamped.dtype == bool and not clamped.any()
    assert np.array_equal(tables, soft) and not np.array_equal(tables, _libjpeg_pair(30))      # real against integer division
    for subsampling, optimize in (('4:4:4', False), ('4:2:0', True)):
        y, sizes, files = model.process_files(x, subsampling=subsampling, optimize=optimize, return_files=True)
        want, want_sizes = jh.compress_batch(x, None, subsampling=subsampling, optimize=optimize, qtables=tables)
        assert y.dtype == np.float32 and np.array_equal(_bits(y), _bits(want)) and sizes == want_sizes == [len(f) for f in files]
        for f in files:
            assert np.array_equal(jh.parse_header(f).qtables, qref.per_component(soft))
        assert np.array_equal(_bits(jh.decode_batch(files, as_float=True)), _bits(y))
    assert len(model.process_files(x)) == 2
    tables, clamped = JPEG(quality=None, codec='sin', device=dev).file_tables()          # no quality: the codec divides by ones
    assert np.array_equal(tables, np.ones((2, 64))) and not clamped.any()
    with pytest.raises(NotImplementedError):
        model.process_files(torch.from_numpy(x).to(dev).requires_grad_())


def test_model_with_learned_tables(dev):
    from neural_imaging_amd.models.jpeg import JPEG
    x = _sources(2, 17, 33).astype(np.float32) / np.float32(255)
    model = JPEG(quality=50, codec='soft', trainable=True, device=dev)
    rng = np.random.default_rng(5)
    w = (0.37 * np.stack([jh.jpeg_qtable(50, 0).ravel(), jh.jpeg_qtable(50, 1).ravel()]) + rng.normal(0, 2, (2, 64))).astype(np.float32)
    w[0, 0], w[0, 1], w[1, 63], w[1, 5], w[1, 6] = 0.3, 2.5, 260.25, 3.5, -1.0       # below 1 | ties | above 255 | negative
    model._codec_model.params.flat.copy_(torch.from_numpy(w.reshape(-1)))
    tables, clamped = model.file_tables()
    want, status = qref.tables_from_float(w[None])
    assert status.tolist() == [3] and np.array_equal(tables, want[0, :2]) and np.array_equal(clamped, qref.moved(w))
    assert tables[0, 0] == 1 and tables[0, 1] == 2 and tables[1, 63] == 255 and tables[1, 5] == 4 and tables[1, 6] == 1
    assert clamped.sum() >= 3 and clamped[0, 0] and clamped[1, 63] and clamped[1, 6] and not clamped[0, 1]
    y, sizes, files = model.process_files(x, subsampling='4:2:2', return_files=True)
    for f, s in zip(files, sizes):
        assert len(f) == s and np.array_equal(jh.parse_header(f).qtables, want[0])
    assert np.array_equal(_bits(y), _bits(jh.compress_batch(x, None, subsampling='4:2:2', qtables=tables)[0]))
    assert np.array_equal(_bits(y), _bits(jh.decode_batch(files, as_float=True)))


def test_model_with_the_libjpeg_codec(dev):
    from neural_imaging_amd.models.jpeg import JPEG
    x = _sources(2, 24, 40).astype(np.float32) / np.float32(255)
    model = JPEG(quality=49, codec='libjpeg', device=dev)
    tables, clamped = model.file_tables()
    assert np.array_equal(tables, _libjpeg_pair(49)) and tables.dtype == np.uint16 and not clamped.any()
    y, sizes, files = model.process_files(x, return_files=True)
    want, want_sizes = jh.compress_batch(x, 49)
    assert np.array_equal(_bits(y), _bits(want)) and sizes == want_sizes and files == jh.encode_batch(x, 49)
    assert np.array_equal(_bits(model.process(x).numpy()), _bits(y))
    with pytest.raises(ValueError):
        JPEG(quality=(30, 90), codec='libjpeg', device=dev).file_tables()
