"""JPEG files with optimised Huffman tables on the GPU (csrc/jpegc_opt.hip through ops.jpeg_histogram / jpeg_optimal_tables /
jpeg_encode_tables and the optimize=True paths of compression.jpeg_helpers): histograms, tables, entropy-coded bytes and whole files
against the plain Python restatement (tests/jpegopt_ref.py), the host program over csrc/jpegopt.h and Pillow's golden files -
everything exact, nothing has a tolerance."""
import os

import numpy as np
import pytest
import torch

import jpeg_cases
import jpegd_cases
import jpegopt_cases as cases
import jpegopt_ref as oref
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


def _coefficients(case, dev):
    hs, vs = ops.jpeg_subsampling(case.subsampling)
    x = torch.from_numpy(np.array(cases.build(case))).to(dev)
    return ops.jpeg_transform(x, case.quality, hs, vs), hs, vs


def _encode_tables(coef, tables, h, w, hs, vs, dev, capacity=None):
    """-> ([segment bytes], lengths, status) with canaries around the output and the workspace checked; nothing at or beyond
    `capacity` may be written."""
    from neural_imaging_amd import _lib
    n = coef.shape[0]
    bound = n * ops.jpeg_ecd_bound_tables(h, w, hs, vs)
    ws_all, ws = _guarded((int(_lib.load().nimg_jpeg_encode_tables_workspace_bytes(n, h, w, hs, vs)),), torch.uint8, 0xa5, dev)
    out_all, out = _guarded((bound,), torch.uint8, 0x5a, dev)
    tables = torch.from_numpy(np.array(tables, order='C')).to(dev) if not isinstance(tables, torch.Tensor) else tables
    data, lengths, status = ops.jpeg_encode_tables(coef, tables, h, w, hs, vs, out=out, workspace=ws, capacity=capacity)
    lengths, status, blob = lengths.cpu().numpy().astype(np.int64), status.cpu().numpy().astype(np.int64), data.cpu().numpy()
    assert _intact(ws_all, 0xa5), 'a write outside the workspace'
    assert _intact(out_all, 0x5a), 'a write outside the output'
    written = min(int(lengths.sum()), bound if capacity is None else capacity)
    assert (blob[written:] == 0x5a).all(), 'a write behind the last segment or beyond the capacity'
    ends = np.concatenate([[0], np.cumsum(lengths)])
    return [blob[ends[i]:min(ends[i + 1], written)].tobytes() for i in range(n)], lengths, status


# ---- 1. every stage, every case ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', cases.CASES, ids=cases.IDS)
def test_every_stage_equals_the_restatement(dev, case):
    r = cases.reference(case)
    coef, hs, vs = _coefficients(case, dev)
    n = coef.shape[0]
    assert np.array_equal(coef.cpu().numpy().reshape(n, -1), r.flat), 'coefficients'
    hist_all, hist = _guarded((n, 4, 257), torch.int32, 0x77, dev)
    ops.jpeg_histogram(coef, case.h, case.w, hs, vs, out=hist)
    assert _intact(hist_all, 0x77)
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), r.hists), 'histograms'
    tables, status = ops.jpeg_optimal_tables(hist)
    assert not status.cpu().numpy().any() and np.array_equal(tables.cpu().numpy(), r.tables), 'tables'
    segments, lengths, status = _encode_tables(coef, tables, case.h, case.w, hs, vs, dev)
    assert not status.any() and segments == r.ecds, 'entropy-coded bytes'
    files = jh.encode_batch(cases.build(case), case.quality, case.subsampling, optimize=True)
    assert files == r.files
    if case.golden:
        assert files == cases.golden()[case.name], 'not the file libjpeg writes with optimize_coding'


@pytest.mark.parametrize('name', ['noise+smooth+constant+checker_16x24_q75_422', 'smooth+noise+half_13x21_q95_420',
                                  'noise+mixed_128x192_q30_420'])
def test_image_in_a_batch_equals_image_alone(dev, name):
    case = cases.by_name(name)
    x = cases.build(case)
    coef, hs, vs = _coefficients(case, dev)
    together = ops.jpeg_optimal_tables(ops.jpeg_histogram(coef, case.h, case.w, hs, vs))[0].cpu().numpy()
    files = jh.encode_batch(x, case.quality, case.subsampling, optimize=True)
    for i in range(len(x)):
        alone = ops.jpeg_optimal_tables(ops.jpeg_histogram(coef[i:i + 1].contiguous(), case.h, case.w, hs, vs))[0].cpu().numpy()
        assert np.array_equal(alone[0], together[i])
        assert jh.encode_batch(x[i], case.quality, case.subsampling, optimize=True) == [files[i]]
    assert len({t.tobytes() for t in together}) == len(together)              # the tables differ between the images of one launch


# ---- 2. the table construction on synthetic histograms -------------------------------------------------------------------------
def test_synthetic_histograms(dev):
    names, hists = cases.synthetic()
    want_tables, want_status = cases.synthetic_reference()
    host_tables, host_status, _, _, done = cases.host_results(hists, [], [], sanitize=False)
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    assert np.array_equal(host_tables, want_tables) and np.array_equal(host_status, want_status)
    h = torch.from_numpy(hists.view(np.int32).copy()).to(dev)
    m = len(names)
    tab_all, tables = _guarded((m, 272), torch.uint8, 0x3c, dev)
    st_all, status = _guarded((m,), torch.int32, 0x3c, dev)
    from neural_imaging_amd import _lib
    _lib.call('nimg_jpeg_optimal_tables', h.data_ptr(), m, tables.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert _intact(tab_all, 0x3c) and _intact(st_all, 0x3c)
    got, st = tables.cpu().numpy(), status.cpu().numpy()
    for k, name in enumerate(names):
        assert st[k] == want_status[k] and np.array_equal(got[k], want_tables[k]), name
    one = ops.jpeg_optimal_tables(h[5:6].contiguous())                          # fibonacci-30: one table, three idle waves
    assert np.array_equal(one[0].cpu().numpy(), want_tables[5:6]) and one[1].cpu().numpy().tolist() == [0]
    some = ops.jpeg_optimal_tables(h[:65].contiguous())                         # 65 tables: a last workgroup with one table
    assert np.array_equal(some[0].cpu().numpy(), want_tables[:65]) and np.array_equal(some[1].cpu().numpy(), want_status[:65])
    grouped = ops.jpeg_optimal_tables(h[:64].view(16, 4, 257))                  # leading dimensions are kept
    assert tuple(grouped[0].shape) == (16, 4, 272) and np.array_equal(grouped[0].cpu().numpy().reshape(64, 272), want_tables[:64])


# ---- 3. coding with the tables of a file: a bit-exact transcode ----------------------------------------------------------------
def _transcode_files():
    out = []
    for name, files in cases.golden().items():
        out += [('{}/{}'.format(name, i), f) for i, f in enumerate(files)]
    return out + [(f.name, f.data) for f in jpegd_cases.foreign_files()]


def test_transcode_reproduces_the_entropy_coded_segment(dev):
    files = _transcode_files()
    assert len(files) == 47 + len(jpegd_cases.FOREIGN)
    for name, data in files:
        hd = jh.parse_header(data)
        assert hd.huffman[4:] == hd.huffman[2:4], name                       # Cb and Cr share their tables
        tables = np.stack([oref.table_of(c, s) for c, s in hd.huffman[:4]])[None]
        coef, _ = jh.decode_coefficients(data, device_output=True)
        segments, lengths, status = _encode_tables(coef, tables, hd.h, hd.w, hd.hs, hd.vs, dev)
        assert status.tolist() == [0] and segments == [data[hd.ecd_offset:hd.ecd_end]], name


@pytest.mark.parametrize('name', ['noise+smooth+constant+checker_16x24_q75_422', 'noise+mixed_128x192_q30_420', 'noise_1x1_q95_420'])
def test_annex_k_tables_give_the_baseline_segments(dev, name):
    case = cases.by_name(name)
    coef, hs, vs = _coefficients(case, dev)
    n = coef.shape[0]
    segments, lengths, status = _encode_tables(coef, np.broadcast_to(oref.ANNEX_K, (n, 4, 272)), case.h, case.w, hs, vs, dev)
    data, want = ops.jpeg_encode(coef, case.h, case.w, hs, vs)
    want = want.cpu().numpy().astype(np.int64)
    assert not status.any() and lengths.tolist() == want.tolist()
    assert b''.join(segments) == data[:int(want.sum())].cpu().numpy().tobytes() == b''.join(jpeg_cases.reference(case).ecds)


# ---- 4. status bits, canaries, capacity ----------------------------------------------------------------------------------------
def test_status_bits(dev):
    case = cases.by_name('noise+smooth+constant+checker_16x24_q75_422')
    r = cases.reference(case)
    coef, hs, vs = _coefficients(case, dev)
    tables = r.tables.copy()
    tables[0] = r.tables[2]                          # the noise image with the tables of the constant one: valid, most symbols missing
    tables[1, 1, 1] = 5                              # five codes of two bits: no prefix code
    want0, st0 = oref.entropy_code(r.coefs[0], case.h, case.w, hs, vs, tables[0])
    assert st0 == oref.ST_SYMBOL and oref.entropy_code(r.coefs[1], case.h, case.w, hs, vs, tables[1]) == (b'', oref.ST_TABLE)
    segments, lengths, status = _encode_tables(coef, tables, case.h, case.w, hs, vs, dev)
    assert status.tolist() == [oref.ST_SYMBOL, oref.ST_TABLE, 0, 0]
    assert segments == [want0, b'', r.ecds[2], r.ecds[3]] and lengths.tolist() == [len(want0), 0, len(r.ecds[2]), len(r.ecds[3])]
    # every other way a table set is refused, and tables that name more than the coder can use
    for bad in ((0, 0, 3), (3, 15, 255), (2, 7, 255)):
        tables = r.tables.copy()
        tables[0, bad[0], bad[1]] = bad[2]
        segments, lengths, status = _encode_tables(coef, tables, case.h, case.w, hs, vs, dev)
        assert status.tolist() == [oref.ST_TABLE, 0, 0, 0] and segments == [b''] + r.ecds[1:], bad
    tables = r.tables.copy()
    tables[2] = 0                                    # no codes at all: valid, every symbol missing, only the padding is left
    segments, lengths, status = _encode_tables(coef, tables, case.h, case.w, hs, vs, dev)
    assert status.tolist() == [0, 0, oref.ST_SYMBOL, 0] and segments == r.ecds[:2] + [b''] + r.ecds[3:]
    # the helpers name the images and the bits
    with pytest.raises(ValueError, match=r'image\(s\) \[1, 3\].*1: status 1 \(Huffman table that is no prefix code\).*3: status 10'):
        jh._raise_on_opt_status(np.array([0, 1, 0, 10]))


def test_longest_codes_fit_the_slot(dev):
    """Every code 16 bits long and every coefficient at its clamp: 1665 bits a block, more than the Annex K bound of 1658."""
    h = w = 16
    nb = ops.jpeg_geometry(h, w, 1, 1)[0]
    coef = torch.full((1, nb, 64), 1023, dtype=torch.int16, device=dev)
    coef[0, :, 0] = torch.tensor([2047, -2047] * (nb // 2), dtype=torch.int16, device=dev)
    coefs = [c.reshape(2, 2, 64) for c in coef[0].cpu().numpy().reshape(3, 4, 64)]
    table = np.zeros(272, np.uint8)
    table[15] = 2                                    # two codes of 16 bits: the DC category 11 / the AC symbol 0A, and one more
    tables = np.stack([table] * 4)
    tables[0::2, 16:18] = (11, 0)
    tables[1::2, 16:18] = (0x0a, 0)
    want, st = oref.entropy_code(coefs, h, w, 1, 1, tables)
    assert st == 0 and len(want.replace(b'\xff\x00', b'\xff')) == -(-12 * 1665 // 8)
    segments, lengths, status = _encode_tables(coef, tables[None], h, w, 1, 1, dev)
    assert status.tolist() == [0] and segments == [want]


def test_nothing_is_written_beyond_the_capacity(dev):
    case = cases.by_name('noise+smooth+constant+checker_16x24_q75_422')
    r = cases.reference(case)
    coef, hs, vs = _coefficients(case, dev)
    want = b''.join(r.ecds)
    for short in (1, 2, len(r.ecds[-1]) + 3, len(want) - 8, len(want) - 1):
        segments, lengths, status = _encode_tables(coef, r.tables, case.h, case.w, hs, vs, dev, capacity=len(want) - short)
        assert lengths.tolist() == [len(e) for e in r.ecds] and not status.any()      # the lengths still say what is needed
        assert b''.join(segments) == want[:len(want) - short]


def test_a_batch_given_too_little_is_coded_again(dev, monkeypatch):
    case = cases.by_name('noise+smooth+constant+checker_16x24_q75_422')
    monkeypatch.setattr(ops, 'jpeg_ecd_bound_tables', lambda *a: 16)
    assert jh.encode_batch(cases.build(case), case.quality, case.subsampling, optimize=True) == cases.reference(case).files


# ---- 5. the Python surface -------------------------------------------------------------------------------------------------------
def test_compress_batch(dev):
    case = cases.by_name('smooth+noise+half_13x21_q95_420')
    x, r = cases.build(case), cases.reference(case)
    sizes = [len(f) for f in r.files]
    for batch in (x, x.astype(np.float32) / np.float32(255)):
        plain, plain_sizes = jh.compress_batch(batch, case.quality, subsampling=case.subsampling)
        y, b = jh.compress_batch(batch, case.quality, subsampling=case.subsampling, optimize=True)
        assert y.dtype == np.float32 and np.array_equal(y.view(np.uint32), plain.view(np.uint32))
        assert b == sizes and all(s < p for s, p in zip(b, plain_sizes))
        assert jh.compress_batch(batch, case.quality, True, case.subsampling, optimize=True)[1] == [s - 177 for s in sizes]
        y1, b1 = jh.compress_batch(batch[1], case.quality, subsampling=case.subsampling, optimize=True)
        assert isinstance(b1, int) and b1 == sizes[1] and np.array_equal(y1, jh.compress_batch(batch[1], case.quality, subsampling=case.subsampling)[0])
    files = jh.encode_batch(x, case.quality, case.subsampling, optimize=True)
    assert [jh.JPEGMarkerStats(f).get_effective_bytes() for f in files] == [s - 177 for s in sizes]
    assert np.array_equal(jh.decode_batch(files), jh.decode_batch(jh.encode_batch(x, case.quality, case.subsampling)))
    image, segments, tables = jh.device_codec(torch.from_numpy(np.array(x)).to(dev), case.quality, case.subsampling, optimize=True)
    assert segments == r.ecds and np.array_equal(tables, r.tables) and image.shape == x.shape
    assert len(jh.device_codec(torch.from_numpy(np.array(x)).to(dev), case.quality, case.subsampling)) == 2


def test_rate_distortion(dev):
    x = ratedist_cases.rd_images(176, 192)[:2]
    qualities = (30, 75, 95)
    for subsampling, effective in (('4:2:0', True), ('4:4:4', False)):
        plain = jh.rate_distortion(x, qualities, subsampling=subsampling, effective=effective)
        out = jh.rate_distortion(x, qualities, subsampling=subsampling, effective=effective, optimize=True)
        for k, q in enumerate(qualities):
            files = jh.encode_batch(x, q, subsampling, optimize=True)
            assert out['bytes'][k].tolist() == [len(f) - (177 if effective else 0) for f in files], (subsampling, q)
        assert np.array_equal(out['bpp'], 8 * out['bytes'] / 176 / 192) and (out['bytes'] < plain['bytes']).all()
        for key in ('ssim', 'psnr', 'msssim', 'msssim_db'):
            assert np.array_equal(out[key], plain[key]), key


def test_match_quality_batch_equals_match_quality_per_image(dev):
    x = ratedist_cases.match_images()[:2]
    target = [8 * jh.compress_batch(x[i], q, optimize=True)[1] / 64 / 72 + 0.003 for i, q in enumerate((37, 62))]
    got = jh.match_quality_batch(x, target, match='bpp', optimize=True)
    want = [jh.match_quality(x[i], target[i], match='bpp', optimize=True) for i in range(2)]
    assert got.tolist() == want and all(1 <= q <= 95 for q in want)


def test_get_jpeg_df(dev, tmp_path):
    pytest.importorskip('pandas')
    from neural_imaging_amd.compression import ratedistortion as rd
    x = ratedist_cases.write_pngs(tmp_path)
    with open(os.path.join(str(tmp_path), 'jpeg.csv'), 'w') as f:
        f.write('not a table: never read, never rewritten\n')
    df = rd.get_jpeg_df(str(tmp_path), optimize=True)
    assert open(os.path.join(str(tmp_path), 'jpeg.csv')).read() == 'not a table: never read, never rewritten\n'
    assert os.path.isfile(os.path.join(str(tmp_path), 'jpeg-optimized.csv'))
    qualities = list(range(95, 5, -5))
    want = jh.rate_distortion(x, qualities, optimize=True)
    assert df['bytes'].tolist() == want['bytes'].T.reshape(-1).tolist() and df['quality'].tolist() == qualities * 3
    again = rd.get_jpeg_df(str(tmp_path), optimize=True)                 # the cached file
    assert again['bytes'].tolist() == df['bytes'].tolist() and again['ssim'].tolist() == df['ssim'].tolist()
    os.remove(os.path.join(str(tmp_path), 'jpeg.csv'))
    plain = rd.get_jpeg_df(str(tmp_path))
    assert (plain['bytes'].to_numpy() > df['bytes'].to_numpy()).all()
