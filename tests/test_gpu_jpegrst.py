"""JPEG files with restart intervals on the GPU: the writer (ops.jpeg_encode / jpeg_histogram /
jpeg_encode_tables with restart_interval=, and encode_batch / compress_batch above them) byte for byte against Pillow's golden files,
the reader (ops.jpeg_decode with restart_interval=, decode_batch / decode_coefficients / transcode_batch with allow_restart=) against
Pillow's decoded bytes, the restatement (tests/jpegrst_ref.py) and the sanitized host program (tests/jpegrst_host.cpp) - everything
exact, nothing has a tolerance."""
import numpy as np
import pytest
import torch

import jpeg_ref as ref
import jpegrst_cases as cases
import jpegrst_ref as rref
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


def _guarded(size, fill, dev):
    """(the whole buffer, a view of `size` bytes with GUARD canary bytes in front of it and behind it)."""
    whole = torch.full((size + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
    return whole, whole[GUARD:GUARD + size]


def _intact(whole, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


def _lib():
    from neural_imaging_amd import _lib
    return _lib


def _coefficients(case, dev, variant='plain'):
    flat = np.stack([ref.flat_coefficients(c) for c in cases.coefficients(case, variant)])
    return torch.from_numpy(flat.reshape(len(flat), -1, 64)).to(dev)


def _segments(files):
    return [f[rref.parse(f)['ecd_offset']:-2] for f in files]


def _split(blob, lengths, written):
    ends = np.concatenate([[0], np.cumsum(lengths)])
    return [blob[ends[i]:min(ends[i + 1], written)].tobytes() for i in range(len(lengths))]


# ---- 1. the writer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', cases.CASES, ids=cases.IDS)
def test_files_are_pillows(dev, case):
    x, g = cases.build(case), cases.golden()[case.name]
    for variant in case.variants:
        ri, optimize, qt = cases.variant_settings(case, variant)
        files = jh.encode_batch(x, None if qt is not None else case.quality, case.subsampling, optimize=optimize, qtables=qt,
                                restart_interval=ri)
        assert files == g.files[variant], variant
    assert jh.encode_batch(x[1], case.quality, case.subsampling, restart_interval=case.ri) == [g.files['plain'][1]]      # one image


@pytest.mark.parametrize('name', ['mixed+noise+smooth_40x56_q75_420_ri5', 'mixed+noise_24x40_q50_422_ri2', 'noise+mixed_16x48_q90_444_ri1'])
def test_compress_batch_counts_the_files(dev, name):
    case = cases.by_name(name)
    x, g = cases.build(case), cases.golden()[case.name]
    today = jh.compress_batch(x, case.quality, subsampling=case.subsampling)[0]
    for variant in case.variants:
        ri, optimize, qt = cases.variant_settings(case, variant)
        how = dict(subsampling=case.subsampling, optimize=optimize, qtables=qt, restart_interval=ri)
        image, sizes = jh.compress_batch(x, None if qt is not None else case.quality, **how)
        assert sizes == [len(f) for f in g.files[variant]], variant
        effective = jh.compress_batch(x, None if qt is not None else case.quality, effective=True, **how)[1]
        assert effective == [jh.JPEGMarkerStats(f).get_effective_bytes() for f in g.files[variant]], variant
        if qt is None:
            assert np.array_equal(image, today), variant                   # the image comes from the coefficients: unchanged
    one, size = jh.compress_batch(x[0], case.quality, subsampling=case.subsampling, restart_interval=case.ri)
    assert size == len(g.files['plain'][0]) and np.array_equal(one, jh.compress_batch(x[0], case.quality, subsampling=case.subsampling)[0])


def _encode(coef, case, ri, dev, capacity=None, tables=None):
    """ops.jpeg_encode / jpeg_encode_tables between canary bytes -> ([segment bytes], lengths); nothing at or beyond `capacity` may be
    written."""
    hs, vs = ops.jpeg_subsampling(case.subsampling)
    n, lib = coef.shape[0], _lib().load()
    if tables is None:
        need = lib.nimg_jpeg_encode_restart_workspace_bytes(n, case.h, case.w, hs, vs, ri) if ri else \
            lib.nimg_jpeg_workspace_bytes(n, case.h, case.w, hs, vs)
        bound = n * ops.jpeg_ecd_bound(case.h, case.w, hs, vs, ri)
    else:
        need = lib.nimg_jpeg_encode_tables_restart_workspace_bytes(n, case.h, case.w, hs, vs, ri) if ri else \
            lib.nimg_jpeg_encode_tables_workspace_bytes(n, case.h, case.w, hs, vs)
        bound = n * ops.jpeg_ecd_bound_tables(case.h, case.w, hs, vs, ri)
    ws_all, ws = _guarded(int(need), 0xa5, dev)
    out_all, out = _guarded(bound, 0x5a, dev)
    if tables is None:
        data, lengths = ops.jpeg_encode(coef, case.h, case.w, hs, vs, out=out, workspace=ws, capacity=capacity, restart_interval=ri)
    else:
        data, lengths, status = ops.jpeg_encode_tables(coef, tables, case.h, case.w, hs, vs, out=out, workspace=ws, capacity=capacity,
                                                       restart_interval=ri)
        assert not status.cpu().numpy().any()
    lengths, blob = lengths.cpu().numpy().astype(np.int64), data.cpu().numpy()
    assert _intact(ws_all, 0xa5), 'a write outside the workspace'
    assert _intact(out_all, 0x5a), 'a write outside the output'
    written = min(int(lengths.sum()), bound if capacity is None else capacity)
    assert (blob[written:] == 0x5a).all(), 'a write behind the last segment or beyond the capacity'
    return _split(blob, lengths, written), lengths


@pytest.mark.parametrize('case', cases.CASES, ids=cases.IDS)
def test_segments_between_canaries_and_a_capacity_one_byte_short(dev, case):
    hs, vs = ops.jpeg_subsampling(case.subsampling)
    coef = _coefficients(case, dev)
    g = cases.golden()[case.name]
    want = _segments(g.files['plain'])
    segments, lengths = _encode(coef, case, case.ri, dev)
    assert segments == want and lengths.tolist() == [len(s) for s in want]
    short, needed = _encode(coef, case, case.ri, dev, capacity=int(lengths.sum()) - 1)
    assert needed.tolist() == lengths.tolist()                             # `lengths` reports what was needed
    assert b''.join(short) == b''.join(want)[:-1]
    # the histograms libjpeg's statistics pass counts, their tables, and the segments coded with them
    hist = ops.jpeg_histogram(coef, case.h, case.w, hs, vs, restart_interval=case.ri)
    assert np.array_equal(hist.cpu().numpy().view(np.uint32),
                          np.stack([rref.histograms(c, case.h, case.w, hs, vs, case.ri) for c in cases.coefficients(case)]))
    tables, status = ops.jpeg_optimal_tables(hist)
    assert not status.cpu().numpy().any() and np.array_equal(tables.cpu().numpy(), np.stack(cases.restated(case, 'opt').huffman))
    want = _segments(g.files['opt'])
    segments, lengths = _encode(coef, case, case.ri, dev, tables=tables)
    assert segments == want
    short, needed = _encode(coef, case, case.ri, dev, capacity=int(lengths.sum()) - 1, tables=tables)
    assert needed.tolist() == lengths.tolist() and b''.join(short) == b''.join(want)[:-1]


def test_interval_zero_through_the_new_entry_points_is_todays_output(dev):
    lib, stream = _lib(), torch.cuda.current_stream().cuda_stream
    for name in ('mixed+noise+smooth_40x56_q75_420_ri5', 'noise+mixed_16x48_q90_444_ri1'):
        case = cases.by_name(name)
        hs, vs = ops.jpeg_subsampling(case.subsampling)
        coef = _coefficients(case, dev)
        n = coef.shape[0]
        today, lengths = _encode(coef, case, 0, dev)
        for new, old in (('nimg_jpeg_encode_restart_workspace_bytes', 'nimg_jpeg_workspace_bytes'),
                         ('nimg_jpeg_encode_tables_restart_workspace_bytes', 'nimg_jpeg_encode_tables_workspace_bytes')):
            assert getattr(lib.load(), new)(n, case.h, case.w, hs, vs, 0) == getattr(lib.load(), old)(n, case.h, case.w, hs, vs)
        need = max(lib.load().nimg_jpeg_encode_restart_workspace_bytes(n, case.h, case.w, hs, vs, 0),
                   lib.load().nimg_jpeg_encode_tables_restart_workspace_bytes(n, case.h, case.w, hs, vs, 0))
        ws = torch.empty(int(need), dtype=torch.uint8, device=dev)
        out_all, out = _guarded(n * ops.jpeg_ecd_bound(case.h, case.w, hs, vs), 0x5a, dev)
        got = torch.empty(n, dtype=torch.int32, device=dev)
        lib.call('nimg_jpeg_encode_restart', coef.data_ptr(), n, case.h, case.w, hs, vs, 0, out.data_ptr(), out.numel(), got.data_ptr(),
                 ws.data_ptr(), ws.numel(), stream)
        assert got.cpu().numpy().tolist() == lengths.tolist() and _intact(out_all, 0x5a)
        assert _split(out.cpu().numpy(), lengths, int(lengths.sum())) == today
        hist = torch.empty((n, 4, 257), dtype=torch.int32, device=dev)
        lib.call('nimg_jpeg_histogram_restart', coef.data_ptr(), n, case.h, case.w, hs, vs, 0, hist.data_ptr(), stream)
        assert torch.equal(hist, ops.jpeg_histogram(coef, case.h, case.w, hs, vs))
        tables = ops.jpeg_optimal_tables(hist)[0]
        today, lengths = _encode(coef, case, 0, dev, tables=tables)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        out.fill_(0x5a)
        lib.call('nimg_jpeg_encode_tables_restart', coef.data_ptr(), n, case.h, case.w, hs, vs, 0, tables.data_ptr(), out.data_ptr(),
                 out.numel(), got.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        assert got.cpu().numpy().tolist() == lengths.tolist() and not status.cpu().numpy().any() and _intact(out_all, 0x5a)
        assert _split(out.cpu().numpy(), lengths, int(lengths.sum())) == today
        if 'baseopt' in case.variants:
            assert today == _segments(cases.golden()[case.name].files['baseopt'])
        with pytest.raises(RuntimeError, match='NIMG_ERR_ARG'):
            lib.call('nimg_jpeg_encode_restart', coef.data_ptr(), n, case.h, case.w, hs, vs, 65536, out.data_ptr(), out.numel(),
                     got.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    with pytest.raises(ValueError, match='restart_interval'):
        jh.encode_batch(cases.build(case), case.quality, case.subsampling, restart_interval=65536)


# ---- 2. the reader ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', cases.CASES, ids=cases.IDS)
def test_decode_batch_equals_pillow(dev, case):
    g = cases.golden()[case.name]
    for subseq_bits in (32, 256, 2048, 0):
        for variant in ('plain', 'opt'):
            got = jh.decode_batch(g.files[variant], subseq_bits=subseq_bits, allow_restart=True)
            assert got.dtype == np.uint8 and np.array_equal(got, g.rgb), (variant, subseq_bits)
    for variant in case.variants:
        coef, qtables = jh.decode_coefficients(g.files[variant], allow_restart=True)
        parsed = [rref.parse(f) for f in g.files[variant]]
        assert np.array_equal(coef.reshape(len(parsed), -1), np.stack([ref.flat_coefficients(p['coefs']) for p in parsed])), variant
        assert np.array_equal(qtables, np.stack([p['qtables'] for p in parsed])), variant
    with pytest.raises(ValueError, match='restart interval'):               # the default stays a refusal
        jh.decode_batch(g.files['plain'])


def _decode(streams, subseq_bits, dev):
    """ops.jpeg_decode over streams of one geometry and interval, workspace between canaries -> (coef, status, rounds) as numpy."""
    s0 = streams[0]
    ecd = torch.from_numpy(np.frombuffer(b''.join(s.ecd for s in streams) or b'\0', np.uint8).copy()).to(dev)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s.ecd) for s in streams])]).astype(np.int64)).to(dev)
    huff = torch.from_numpy(np.stack([s.huffman for s in streams])).to(dev)
    lib = _lib().load()
    need = lib.nimg_jpeg_decode_restart_workspace_bytes(len(streams), s0.h, s0.w, s0.hs, s0.vs, s0.ri, ecd.numel(), subseq_bits) if s0.ri \
        else lib.nimg_jpeg_decode_workspace_bytes(len(streams), s0.h, s0.w, s0.hs, s0.vs, ecd.numel(), subseq_bits)
    ws_all, ws = _guarded(int(need), 0xa5, dev)
    coef, status, rounds = ops.jpeg_decode(ecd, off, huff, s0.h, s0.w, s0.hs, s0.vs, subseq_bits=subseq_bits, workspace=ws,
                                           restart_interval=s0.ri)
    out = coef.cpu().numpy(), status.cpu().numpy(), rounds.cpu().numpy()
    assert _intact(ws_all, 0xa5), 'a write outside the workspace'
    return out


def test_status_coefficients_and_rounds_equal_the_host_program(dev):
    """Every golden and damaged stream the sanitized host program has completed cleanly, grouped by geometry and interval so that
    images of different content and damage share a launch."""
    streams, results, recoded, done = cases.host_reference()
    assert done.returncode == 0 and done.stderr == b'', done.stderr.decode()[-4000:]
    groups = {}
    for k, s in enumerate(streams):
        groups.setdefault((s.h, s.w, s.hs, s.vs, s.ri), []).append(k)
    # 13 cases of distinct (geometry, interval), 3 of them also without an interval; the DRI damage adds further intervals
    assert len(streams) > 400 and len(groups) >= 16 and any(key[4] == 0 for key in groups)
    zero_rounds = 0
    for key, idx in groups.items():
        part = [streams[k] for k in idx]
        whole = max(max(32, -(-8 * len(s.ecd) // 32) * 32) for s in part)
        for setting in cases.SETTINGS:
            coef, status, rounds = _decode(part, setting or whole, dev)
            for j, k in enumerate(idx):
                r = results[(k, setting)]
                assert status[j] == r.status, (streams[k].name, setting, status[j], r.status)
                assert np.array_equal(coef[j].reshape(-1), r.coef), (streams[k].name, setting)
                if setting:
                    assert rounds[j] == r.rounds, (streams[k].name, setting, rounds[j], r.rounds)
                    intervals = rref.split_segment(streams[k].ecd)[0] if streams[k].ri and not r.status else None
                    if intervals and all(8 * len(p) <= setting for p in intervals):
                        assert rounds[j] == 0, (streams[k].name, setting)
                        zero_rounds += 1
                else:
                    assert rounds[j] == 0, streams[k].name
    assert zero_rounds > 100


def test_mixed_batches_come_back_in_input_order(dev):
    g = cases.golden()
    a, b, c = (g[n] for n in ('mixed+noise+smooth_40x56_q75_420_ri5', 'mixed+noise+smooth_40x56_q75_420_ri1', 'smooth+noise_13x21_q30_444_ri2'))
    files = [a.files['plain'][0], a.files['base'][1], b.files['opt'][2], c.files['plain'][1], a.files['plain'][2], c.files['base'][0],
             b.files['plain'][0]]
    want = [a.rgb[0], a.rgb[1], b.rgb[2], c.rgb[1], a.rgb[2], c.rgb[0], b.rgb[0]]
    got = jh.decode_batch(files, allow_restart=True)
    assert len(got) == len(want) and all(np.array_equal(p, q) for p, q in zip(got, want))
    same = jh.decode_batch([files[0], files[1], files[2]], allow_restart=True)          # one geometry, three intervals: still a list
    assert all(np.array_equal(p, q) for p, q in zip(same, want[:3]))
    with pytest.raises(ValueError, match='one geometry and restart interval'):
        jh.decode_coefficients(files[:2], allow_restart=True)
    at = files[0].index(b'\xff\xd0', jh.parse_header(files[0], allow_restart=True).ecd_offset) + 2
    damaged = files[0][:at] + b'\xff\xd3' + files[0][at:]                  # a surplus marker behind the first
    with pytest.raises(ValueError, match=r'damaged JPEG data in file\(s\) \[1\].*restart markers missing, surplus or out of sequence'):
        jh.decode_batch([files[4], damaged], allow_restart=True)


# ---- 3. round trips -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['mixed+noise+smooth_40x56_q75_420_ri3', 'mixed+noise_24x40_q50_422_ri2', 'noise+smooth_13x21_q75_420_ri1',
                                  'noise+mixed_128x128_q95_420_ri24'])
def test_round_trips(dev, name):
    case = cases.by_name(name)
    x, g = cases.build(case), cases.golden()[case.name]
    image = jh.compress_batch(x, case.quality, subsampling=case.subsampling, restart_interval=case.ri)[0]
    for optimize in (False, True):
        files = jh.encode_batch(x, case.quality, case.subsampling, optimize=optimize, restart_interval=case.ri)
        assert np.array_equal(jh.decode_batch(files, as_float=True, allow_restart=True), image)
    # a foreign file with a DRI segment written again: its interval kept, optimal or Annex K tables
    assert jh.transcode_batch(g.files['plain'], allow_restart=True, optimize=True) == g.files['opt']
    assert jh.transcode_batch(g.files['opt'], allow_restart=True, optimize=False) == \
        jh.encode_batch(x, case.quality, case.subsampling, restart_interval=case.ri) == g.files['plain']
    with pytest.raises(ValueError, match='restart interval'):
        jh.transcode_batch(g.files['plain'])
