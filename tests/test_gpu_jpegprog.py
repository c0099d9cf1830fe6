"""Progressive JPEG files on the GPU (csrc/jpegc_prog.hip through ops.jpeg_progressive_histogram / jpeg_encode_progressive and the
progressive=True paths of compression.jpeg_helpers): histograms, tables, the ten entropy-coded segments and whole files against the
plain Python restatement (tests/jpegprog_ref.py), the host program over csrc/jpegprog.h and Pillow's golden files - everything exact,
nothing has a tolerance."""
import numpy as np
import pytest
import torch

import jpeg_cases
import jpeg_ref as ref
import jpegopt_ref as oref
import jpegprog_cases as cases
import jpegprog_ref as pref
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


@pytest.fixture(scope='module')
def host():
    """case name -> [HostImage per image]: the host program over csrc/jpegprog.h, run once for all cases."""
    images, names = [], []
    for case in cases.CASES:
        hs, vs = ref.SUBSAMPLING[case.subsampling]
        for coef in cases.flat(case):
            images.append(cases.Image(case.h, case.w, hs, vs, case.ri, coef, None))
            names.append(case.name)
    out, done = cases.host_results(images, sanitize=False)
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    result = {}
    for name, o in zip(names, out):
        result.setdefault(name, []).append(o)
    return result


def _guarded(shape, dtype, fill, dev):
    """(the whole buffer as bytes, a view of `shape` with GUARD canary bytes in front of it and behind it)."""
    size = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    whole = torch.full((size + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
    return whole, whole[GUARD:GUARD + size].view(dtype).view(shape)


def _intact(whole, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


def _encode(coef, tables, h, w, hs, vs, dev, ri=0, capacity=None):
    """-> ([[ten segments] per image], lengths (n, 10), status) through the C entry point, with canaries around the output, the lengths
    and the workspace checked; nothing at or beyond `capacity` may be written."""
    from neural_imaging_amd import _lib
    n = coef.shape[0]
    bound = n * ops.jpeg_progressive_ecd_bound(h, w, hs, vs, ri)
    need = int(_lib.load().nimg_jpeg_progressive_workspace_bytes(n, h, w, hs, vs, ri))
    assert need > 0
    ws_all, ws = _guarded((need,), torch.uint8, 0xa5, dev)
    out_all, out = _guarded((bound,), torch.uint8, 0x5a, dev)
    len_all, lengths = _guarded((n, 10), torch.int32, 0x3c, dev)
    st_all, status = _guarded((n,), torch.int32, 0x3c, dev)
    tables = torch.from_numpy(np.array(tables, order='C')).to(dev) if not isinstance(tables, torch.Tensor) else tables.contiguous()
    _lib.call('nimg_jpeg_encode_progressive', coef.data_ptr(), n, h, w, hs, vs, ri, tables.data_ptr(), out.data_ptr(),
              bound if capacity is None else capacity, lengths.data_ptr(), status.data_ptr(), ws.data_ptr(), need,
              torch.cuda.current_stream().cuda_stream)
    lens, st, blob = lengths.cpu().numpy().astype(np.int64), status.cpu().numpy().astype(np.int64), out.cpu().numpy()
    assert _intact(ws_all, 0xa5), 'a write outside the workspace'
    assert _intact(out_all, 0x5a), 'a write outside the output'
    assert _intact(len_all, 0x3c) and _intact(st_all, 0x3c), 'a write outside the lengths or the status'
    written = min(int(lens.sum()), bound if capacity is None else capacity)
    assert (blob[written:] == 0x5a).all(), 'a write behind the last segment or beyond the capacity'
    ends = np.concatenate([[0], np.cumsum(lens.reshape(-1))])
    return [[blob[ends[10 * i + k]:min(ends[10 * i + k + 1], written)].tobytes() for k in range(10)] for i in range(n)], lens, st


def _histogram(coef, h, w, hs, vs, dev, ri=0):
    n = coef.shape[0]
    hist_all, hist = _guarded((n, 10, 257), torch.int32, 0x77, dev)
    ops.jpeg_progressive_histogram(coef, h, w, hs, vs, out=hist, restart_interval=ri)
    assert _intact(hist_all, 0x77)
    return hist


# ---- 1. every stage, every case ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', cases.CASES, ids=cases.IDS)
def test_every_stage_equals_the_host_program_and_pillow(dev, host, case):
    hs, vs = ref.SUBSAMPLING[case.subsampling]
    golden = cases.golden()[case.name]
    want = host[case.name]
    coef = torch.from_numpy(cases.flat(case)).to(dev).view(len(golden), -1, 64)
    hist = _histogram(coef, case.h, case.w, hs, vs, dev, case.ri)
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), np.stack([o.hist for o in want])), 'histograms'
    tables, status = ops.jpeg_optimal_tables(hist)
    assert not status.cpu().numpy().any(), 'table status'
    segments, lengths, status = _encode(coef, tables, case.h, case.w, hs, vs, dev, case.ri)
    assert not status.any()
    tables = tables.cpu().numpy()
    for i, data in enumerate(golden):
        pillow_tables, pillow_segments = cases.split_file(data)
        assert np.array_equal(tables[i], pillow_tables) and np.array_equal(tables[i], want[i].tables), 'tables'
        assert segments[i] == pillow_segments == want[i].segments, 'entropy-coded segments'
        assert lengths[i].tolist() == [len(s) for s in pillow_segments]
    if not case.slow:
        r = cases.reference(case)
        assert np.array_equal(hist.cpu().numpy().view(np.uint32), r.hists) and segments == r.segments, 'the restatement'
    files = jh.encode_batch(cases.build(case), case.quality, case.subsampling, qtables=cases.qtables(case), restart_interval=case.ri,
                            progressive=True)
    assert files == golden, 'not the file libjpeg writes with jpeg_simple_progression'


@pytest.mark.parametrize('s', cases.synthetic(), ids=[s.name for s in cases.synthetic()])
def test_synthetic_coefficients(dev, s):
    """Values beyond the clamps, zero runs of 16 in front of and behind the last new coefficient of a refine block, blocks of
    correction bits alone."""
    want_hist, want_tables, want_segments, stats = cases.synthetic_reference(s.name)
    if s.name.startswith('synthetic'):
        assert stats['zrl_first'] and stats['zrl_refine'] and stats['refine_tail_run']
    coef = torch.from_numpy(s.flat.copy()).to(dev).view(1, -1, 64)
    hist = _histogram(coef, s.h, s.w, s.hs, s.vs, dev, s.ri)
    assert np.array_equal(hist.cpu().numpy().view(np.uint32)[0], want_hist)
    tables, status = ops.jpeg_optimal_tables(hist)
    assert not status.cpu().numpy().any() and np.array_equal(tables.cpu().numpy()[0], want_tables)
    segments, lengths, status = _encode(coef, tables, s.h, s.w, s.hs, s.vs, dev, s.ri)
    assert status.tolist() == [0] and segments == [want_segments]


def test_image_in_a_batch_equals_image_alone(dev):
    case = cases.by_name('g_noise+smooth+constant+checker_16x24_q75_422')
    x = cases.build(case)
    files = jh.encode_batch(x, case.quality, case.subsampling, progressive=True)
    assert files == cases.golden()[case.name] and len(set(files)) == len(files)
    for i in range(len(x)):
        assert jh.encode_batch(x[i], case.quality, case.subsampling, progressive=True) == [files[i]]


# ---- 2. status bits, the slot bound, capacity, arguments -----------------------------------------------------------------------------
def test_status_bits(dev):
    case = cases.by_name('g_noise+smooth+constant+checker_16x24_q75_422')
    r = cases.reference(case)
    hs, vs = ref.SUBSAMPLING[case.subsampling]
    coef = torch.from_numpy(r.flat).to(dev).view(4, -1, 64)
    items = [pref.all_items(c, case.h, case.w, hs, vs) for c in r.coefs]
    tables = r.tables.copy()
    tables[0] = r.tables[2]                          # the noise image with the tables of the constant one: valid, most symbols missing
    tables[1, 7, 1] = 5                              # five codes of two bits in the table of scan 8: no prefix code
    tables[3, 9] = 0                                 # the last scan without any code: only its padding is left
    want = [pref.segments(it, t) for it, t in zip(items, tables)]
    assert [w[1] for w in want] == [oref.ST_SYMBOL, oref.ST_TABLE, 0, oref.ST_SYMBOL] and want[1][0] == [b''] * 10
    segments, lengths, status = _encode(coef, tables, case.h, case.w, hs, vs, dev)
    assert status.tolist() == [w[1] for w in want] and segments == [w[0] for w in want]
    assert segments[2] == r.segments[2] and segments[3][:9] == r.segments[3][:9] and len(segments[3][9]) < len(r.segments[3][9])
    for bad in ((0, 0, 3), (1, 15, 255), (5, 7, 255)):                      # every other way a table set is refused
        tables = r.tables.copy()
        tables[0, bad[0], bad[1]] = bad[2]
        segments, lengths, status = _encode(coef, tables, case.h, case.w, hs, vs, dev)
        assert status.tolist() == [oref.ST_TABLE, 0, 0, 0] and segments == [[b''] * 10] + r.segments[1:], bad
    # with restart markers a refused image is its markers alone
    rst = cases.by_name('mixed_37x53_q75_420_ri3')
    rr = cases.reference(rst)
    tables = rr.tables.copy()
    tables[0, 0, 0] = 3
    segments, lengths, status = _encode(torch.from_numpy(rr.flat).to(dev).view(1, -1, 64), tables, rst.h, rst.w, 2, 2, dev, 3)
    assert status.tolist() == [oref.ST_TABLE]
    assert segments[0] == pref.segments(pref.all_items(rr.coefs[0], rst.h, rst.w, 2, 2, 3), tables[0])[0]
    assert segments[0][1] == b''.join(bytes([0xff, 0xd0 + k % 8]) for k in range(-(-35 // 3) - 1))       # 5 x 7 luma blocks


def test_longest_codes_fit_the_slot(dev):
    """Every code 16 bits long and every coefficient at its clamp: 27 bits a block in the first DC scan, 63 * 25 in the first scans
    of a whole band; a block of 62 such coefficients and a run is 62 * 25 + 16 here and 14 run bits more at 0x7fff blocks - the 1580
    bits the workspace gives every block of an AC scan."""
    assert ops.JPEG_PROGRESSIVE_DC_BITS_MAX == 16 + 11 and ops.JPEG_PROGRESSIVE_AC_BITS_MAX == 62 * (16 + 9) + 16 + 14 > 63 * (16 + 9)
    h, w = 16, 24
    nb = ops.jpeg_geometry(h, w, 1, 1)[0]
    coef = np.full((nb, 64), 1023, np.int16)
    coef[:, 0] = [2047, -2047] * (nb // 2)
    coef[1::2, 63] = 0                               # every other block ends in a run
    coef[2::3, 1:] = -32768                          # and the clamp from below
    table = np.zeros(272, np.uint8)
    table[15] = 4                                    # four codes of 16 bits: the symbols this tensor emits
    tables = np.stack([table] * 10)
    tables[:2, 16:20] = (11, 10, 0, 1)
    tables[2:, 16:20] = (0x09, 0x08, 0x00, 0x20)
    items = pref.all_items(cases.coefs_of_flat(coef.reshape(-1), h, w, 1, 1), h, w, 1, 1)
    want, st = pref.segments(items, tables)
    assert st == 0
    bits = [sum((16 if it[0] == 'sym' else 0) + it[-1] for it in scan) for scan in items]
    assert bits[0] == 3 * (26 + 5 * 27) and bits[2] == 4 * 1575 + 2 * 1566           # Cr: four whole bands, two blocks that end in a run
    segments, lengths, status = _encode(torch.from_numpy(coef).to(dev)[None], tables[None], h, w, 1, 1, dev)
    assert status.tolist() == [0] and segments == [want]


def test_nothing_is_written_beyond_the_capacity(dev):
    case = cases.by_name('g_noise+smooth+constant+checker_16x24_q75_422')
    r = cases.reference(case)
    hs, vs = ref.SUBSAMPLING[case.subsampling]
    coef = torch.from_numpy(r.flat).to(dev).view(4, -1, 64)
    want = b''.join(b''.join(s) for s in r.segments)
    for short in (1, 2, len(r.segments[-1][-1]) + 3, len(want) - 8, len(want) - 1):
        segments, lengths, status = _encode(coef, r.tables, case.h, case.w, hs, vs, dev, capacity=len(want) - short)
        assert lengths.tolist() == [[len(s) for s in img] for img in r.segments] and not status.any()     # they still say what is needed
        assert b''.join(b''.join(s) for s in segments) == want[:len(want) - short]


def test_a_batch_given_too_little_is_coded_again(dev, monkeypatch):
    case = cases.by_name('g_noise+smooth+constant+checker_16x24_q75_422')
    monkeypatch.setattr(ops, 'jpeg_progressive_ecd_bound', lambda *a: 16)
    assert jh.encode_batch(cases.build(case), case.quality, case.subsampling, progressive=True) == cases.golden()[case.name]


def test_arguments(dev):
    from neural_imaging_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    coef = torch.zeros((1, 12, 64), dtype=torch.int16, device=dev)
    tables = torch.zeros((1, 10, 272), dtype=torch.uint8, device=dev)
    hist_all, hist = _guarded((1, 10, 257), torch.int32, 0x77, dev)
    out_all, out = _guarded((64,), torch.uint8, 0x5a, dev)
    lengths = torch.zeros((1, 10), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    need = int(lib.nimg_jpeg_progressive_workspace_bytes(1, 16, 16, 1, 1, 0))
    ws_all, ws = _guarded((need,), torch.uint8, 0xa5, dev)

    def encode(n=1, h=16, w=16, hs=1, vs=1, ri=0, c=coef, t=tables, o=out, ln=lengths, st=status, wk=ws, wb=need):
        return lib.nimg_jpeg_encode_progressive(c.data_ptr() if c is not None else None, n, h, w, hs, vs, ri,
                                                t.data_ptr() if t is not None else None, o.data_ptr() if o is not None else None, 64,
                                                ln.data_ptr() if ln is not None else None, st.data_ptr() if st is not None else None,
                                                wk.data_ptr() if wk is not None else None, wb, stream)

    assert encode(n=0) == 0 and lib.nimg_jpeg_progressive_histogram(coef.data_ptr(), 0, 16, 16, 1, 1, 0, hist.data_ptr(), stream) == 0
    for bad in (dict(n=-1), dict(n=16384), dict(h=0), dict(w=4097), dict(hs=1, vs=2), dict(hs=3), dict(ri=-1), dict(ri=65536), dict(c=None),
                dict(t=None), dict(o=None), dict(ln=None), dict(st=None), dict(wk=None)):
        assert encode(**bad) == -1, bad
    assert encode(wb=need - 1) == -3
    assert lib.nimg_jpeg_progressive_histogram(coef.data_ptr(), 1, 16, 16, 1, 1, 70000, hist.data_ptr(), stream) == -1
    assert lib.nimg_jpeg_progressive_histogram(None, 1, 16, 16, 1, 1, 0, hist.data_ptr(), stream) == -1
    assert lib.nimg_jpeg_progressive_workspace_bytes(1, 16, 16, 2, 3, 0) == 0 and lib.nimg_jpeg_progressive_workspace_bytes(0, 16, 16, 1, 1, 0) == 0
    torch.cuda.synchronize()
    assert _intact(hist_all, 0x77) and (hist == 0x77777777).all() and _intact(out_all, 0x5a) and (out == 0x5a).all() and _intact(ws_all, 0xa5)
    assert (ws == 0xa5).all(), 'a refused call launched something'
    assert encode() == 0                                                     # and the accepted call: all-zero tables, nothing but padding
    torch.cuda.synchronize()
    assert status.tolist() == [oref.ST_SYMBOL] and _intact(ws_all, 0xa5) and _intact(out_all, 0x5a)
    with pytest.raises(RuntimeError, match='do not match the geometry'):
        ops.jpeg_progressive_histogram(coef, 16, 24, 1, 1)
    with pytest.raises(RuntimeError, match=r'\(1, 10, 272\) uint8 needed'):
        ops.jpeg_encode_progressive(coef, tables[:, :4].contiguous(), 16, 16, 1, 1)


# ---- 3. the Python surface -------------------------------------------------------------------------------------------------------
def test_compress_batch_and_device_codec(dev):
    case = cases.by_name('g_smooth+noise+half_13x21_q95_420')
    x, files = cases.build(case), cases.golden()[case.name]
    sizes = [len(f) for f in files]
    for batch in (x, x.astype(np.float32) / np.float32(255)):
        plain, _ = jh.compress_batch(batch, case.quality, subsampling=case.subsampling)
        y, b = jh.compress_batch(batch, case.quality, subsampling=case.subsampling, progressive=True)
        assert y.dtype == np.float32 and np.array_equal(y.view(np.uint32), plain.view(np.uint32)), 'the decoded image changed'
        assert b == sizes
        assert jh.compress_batch(batch, case.quality, True, case.subsampling, progressive=True)[1] == [s - 177 for s in sizes]
        assert jh.compress_batch(batch, case.quality, subsampling=case.subsampling, progressive=True, optimize=True)[1] == sizes
        y1, b1 = jh.compress_batch(batch[1], case.quality, subsampling=case.subsampling, progressive=True)
        assert isinstance(b1, int) and b1 == sizes[1] and np.array_equal(y1, jh.compress_batch(batch[1], case.quality, subsampling=case.subsampling)[0])
    xd = torch.from_numpy(np.array(x)).to(dev)
    image, segments, tables = jh.device_codec(xd, case.quality, case.subsampling, progressive=True)
    assert [(np.asarray(cases.split_file(f)[0]).tobytes(), cases.split_file(f)[1]) for f in files] == \
        [(t.tobytes(), s) for t, s in zip(tables, segments)]
    assert torch.equal(image, jh.device_codec(xd, case.quality, case.subsampling)[0]) and len(jh.device_codec(xd, case.quality, case.subsampling)) == 2
    for optimize in (False, True):
        assert jh.encode_batch(x, case.quality, case.subsampling, optimize=optimize, progressive=True) == files
    three = cases.by_name('mixed_17x33_three_444_ri2')                        # a third quantisation table: everything 69 bytes later
    got = jh.compress_batch(cases.build(three), None, True, three.subsampling, qtables=cases.qtables(three), restart_interval=2, progressive=True)[1]
    assert got == [len(cases.golden()[three.name][0]) - 246]
    assert jh.jpeg_header(13, 21, 95, '4:2:0', huffman=tables[0], progressive=True) == files[0][:files[0].index(b'\xff\xda') + 14]


def test_transcode_batch(dev):
    """Baseline files in, progressive files out: the lossless jpegtran -progressive."""
    names = ['noise+smooth+constant+checker_16x24_q75_422', 'smooth+noise+half_13x21_q95_420', 'mixed_40x56_q75_420', 'noise_8x8_q1_444']
    names = [n for n in names if n in jpeg_cases.golden()] + [c.name for c in jpeg_cases.GOLDEN_CASES[:6]]
    baseline, want = [], []
    for name in dict.fromkeys(names):
        baseline += jpeg_cases.golden()[name][1]
        want += cases.golden()['g_' + name]
    assert len(baseline) >= 8
    assert jh.transcode_batch(baseline, progressive=True) == want
    assert jh.transcode_batch(baseline, optimize=False, progressive=True) == want
    assert jh.transcode_batch(baseline[0], progressive=True) == [want[0]]
    rst = cases.by_name('mixed_37x53_q75_422_ri7')                          # a file with a restart interval keeps it
    plain = jh.encode_batch(cases.build(rst), rst.quality, rst.subsampling, restart_interval=7)
    assert jh.transcode_batch(plain, allow_restart=True, progressive=True) == cases.golden()[rst.name]
    three = cases.by_name('mixed_40x56_three_422')                          # and one with three quantisation tables its tables
    plain = jh.encode_batch(cases.build(three), None, three.subsampling, qtables=cases.qtables(three))
    assert jh.transcode_batch(plain, progressive=True) == cases.golden()[three.name]
    with pytest.raises(ValueError):
        jh.parse_header(want[0])                                            # reading progressive files stays out
