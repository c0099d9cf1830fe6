"""Grey-scale JPEG files on the GPU: the nimg_jpeg_grey_* entry points through ops and compression.jpeg_helpers
- coefficients, whole files and decoded images byte for byte against the restatement (tests/jpeggrey_ref.py) and Pillow's golden files
in every writer mode; the decoders' coefficients, status and rounds against the sanitized host program (tests/jpeggrey_host.cpp);
progressive files and files that declare the factors 2x2; transcoding; calls that mix colour and grey files; guard bytes around every
output and workspace; every NIMG_ERR_* path with a check that the refused call launched nothing; and what stays out.  Everything is
exact, nothing has a tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import jpeggrey_cases as cases
import jpeggrey_ref as gref
from neural_imaging_amd import ops
from neural_imaging_amd.compression import jpeg_helpers as jh

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xa5
GREY = ops.JPEG_GREY
ERR_ARG, ERR_WORKSPACE = -1, -3
WRITERS = [c for c in cases.CASES if 'plain' in c.variants]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()
    assert (_lib.CONSTANTS['NIMG_ERR_ARG'], _lib.CONSTANTS['NIMG_ERR_WORKSPACE']) == (ERR_ARG, ERR_WORKSPACE)
    return torch.device('cuda', 0)


def _lib():
    from neural_imaging_amd import _lib
    return _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(shape, dtype, dev):
    """(the whole buffer, a view of `shape` and `dtype` with GUARD fill bytes in front of it and behind it); everything is FILL."""
    size = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    whole = torch.full((size + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    return whole, whole[GUARD:GUARD + size].view(dtype).view(shape)


def _intact(whole):
    return bool((whole[:GUARD] == FILL).all()) and bool((whole[-GUARD:] == FILL).all())


def _untouched(whole):
    return bool((whole == FILL).all())


def _images(case, dev, as_float=False):
    x = cases.build(case)[..., None]
    # (byte / 255 in float32 on the host: 255 * that, truncated, is the byte again for every byte)
    return torch.from_numpy(x.astype(np.float32) / np.float32(255) if as_float else x.copy()).to(dev)


def _coef(case, dev):
    return torch.from_numpy(np.ascontiguousarray(np.stack([c.reshape(-1, 64) for c in cases.coefficients(case)]))).to(dev)


def _qtabs(case, n, dev):
    return torch.from_numpy(np.repeat(cases.qtable(case).astype(np.uint16).view(np.int16)[None, None], n, 0)).to(dev)


def _split(blob, lengths):
    ends = np.concatenate([[0], np.cumsum(lengths)])
    return [blob[ends[i]:ends[i + 1]].tobytes() for i in range(len(lengths))]


def _segments(files):
    return [gref.split(f)['segments'][0] for f in files]


# ---- 1. the writer, stage by stage between guard bytes ---------------------------------------------------------------------------------
@pytest.mark.parametrize('case', WRITERS, ids=[c.name for c in WRITERS])
def test_stages_equal_the_restatement_between_guard_bytes(dev, case):
    n, h, w, ri = len(case.contents), case.h, case.w, case.ri
    lib = _lib().load()
    want = _coef(case, dev)
    need = int(lib.nimg_jpeg_grey_workspace_bytes(n, h, w, ri))
    assert need == ops.jpeg_workspace_bytes(n, h, w, *GREY, ri) > 0
    ws_all, ws = _guarded((need,), torch.uint8, dev)
    # the transform: uint8 and float input, a quality or the table itself
    for x in (_images(case, dev), _images(case, dev, as_float=True)):
        got = ops.jpeg_transform_tables(x, _qtabs(case, n, dev), workspace=ws)
        assert torch.equal(got[0], want) and int(got[1]) == 0
        if not case.qt:
            assert torch.equal(ops.jpeg_transform(x, case.quality, workspace=ws), want)
            assert torch.equal(ops.jpeg_transform(x, case.quality, *GREY, workspace=ws), want)
    # the Annex K coder, and a capacity one byte short
    g = cases.golden()[case.name]
    segs = _segments(g.files['plain'])
    bound = n * ops.jpeg_ecd_bound(h, w, *GREY, ri)
    for short in (0, 1):
        out_all, out = _guarded((bound,), torch.uint8, dev)
        capacity = sum(len(s) for s in segs) - short
        data, lengths = ops.jpeg_encode(want, h, w, *GREY, out=out, workspace=ws, capacity=capacity, restart_interval=ri)
        assert lengths.cpu().numpy().tolist() == [len(s) for s in segs]
        blob = data.cpu().numpy()
        assert blob[:capacity].tobytes() == b''.join(segs)[:capacity] and (blob[capacity:] == FILL).all() and _intact(out_all)
    # the two histograms, their tables, the coder with them
    hist_all, hist = _guarded((n, 2, 257), torch.int32, dev)
    ops.jpeg_histogram(want, h, w, *GREY, out=hist, restart_interval=ri)
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), np.stack([gref.histograms(c, ri) for c in cases.coefficients(case)]))
    assert _intact(hist_all)
    if 'opt' in case.variants:
        tables, status = ops.jpeg_optimal_tables(hist)
        assert not status.cpu().numpy().any() and np.array_equal(tables.cpu().numpy(), np.stack(cases.restated(case, 'opt')[1]))
        need_t = int(lib.nimg_jpeg_grey_encode_tables_workspace_bytes(n, h, w, ri))
        wt_all, wt = _guarded((need_t,), torch.uint8, dev)
        out_all, out = _guarded((n * ops.jpeg_ecd_bound_tables(h, w, *GREY, ri),), torch.uint8, dev)
        data, lengths, status = ops.jpeg_encode_tables(want, tables, h, w, *GREY, out=out, workspace=wt, restart_interval=ri)
        lengths = lengths.cpu().numpy()
        assert not status.cpu().numpy().any() and _split(data.cpu().numpy(), lengths) == _segments(g.files['opt'])
        assert _intact(out_all) and _intact(wt_all)
    # the way back: uint8 and float32
    for out_u8 in (True, False):
        y_all, y = _guarded((n, h, w, 1), torch.uint8 if out_u8 else torch.float32, dev)
        ops.jpeg_reconstruct_tables(want, h, w, _qtabs(case, n, dev), *GREY, out_u8=out_u8, workspace=ws, out=y)
        pixels = g.pixels[..., None]
        assert np.array_equal(y.cpu().numpy(), pixels if out_u8 else pixels.astype(np.float32) / np.float32(255)) and _intact(y_all)
    assert _intact(ws_all)


# ---- 2. whole files ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', WRITERS, ids=[c.name for c in WRITERS])
def test_files_are_pillows(dev, case):
    x, g = cases.build(case)[..., None], cases.golden()[case.name]
    how = dict(qtables=cases.QTABLES[case.qt][None]) if case.qt else {}
    quality = None if case.qt else case.quality
    for variant in ('plain', 'opt'):
        if variant in case.variants:
            files = jh.encode_batch(x, quality, optimize=variant == 'opt', restart_interval=case.ri, **how)
            assert files == g.files[variant] == cases.restated(case, variant)[0], variant
    assert jh.encode_batch(x[-1], quality, 'grey', restart_interval=case.ri, **how) == [g.files['plain'][-1]]         # one (h,w,1) image
    assert jh.encode_batch(x.astype(np.float32) / np.float32(255), quality, restart_interval=case.ri, **how) == g.files['plain']
    if case.qt:                                               # two or three tables: the first alone is used, as libjpeg does
        other = cases.QTABLES['ones' if case.qt == 'arb' else 'arb']
        assert jh.encode_batch(x, None, qtables=[cases.QTABLES[case.qt], other], restart_interval=case.ri) == g.files['plain']
        assert jh.encode_batch(x, None, qtables=[cases.QTABLES[case.qt], other, other], restart_interval=case.ri) == g.files['plain']


@pytest.mark.parametrize('name', ['flat+noise+mixed_20x27_q75_ri0', 'noise+mixed_20x27_qt-ones_ri0', 'noise+mixed_20x27_q75_ri5', 'noise_1x1_q75_ri0'])
def test_compress_batch_returns_libjpegs_image_and_counts_the_files(dev, name):
    case = cases.by_name(name)
    x, g = cases.build(case)[..., None], cases.golden()[case.name]
    how = dict(qtables=cases.QTABLES[case.qt][None]) if case.qt else {}
    quality = None if case.qt else case.quality
    want = g.pixels[..., None].astype(np.float32) / np.float32(255)
    for variant in ('plain', 'opt'):
        image, sizes = jh.compress_batch(x, quality, optimize=variant == 'opt', restart_interval=case.ri, **how)
        assert image.dtype == np.float32 and np.array_equal(image, want) and sizes == [len(f) for f in g.files[variant]], variant
        effective = jh.compress_batch(x, quality, effective=True, optimize=variant == 'opt', restart_interval=case.ri, **how)[1]
        assert effective == [len(f) - f.index(b'\xff\xc4') for f in g.files[variant]] == [s - 102 for s in sizes], variant
    one, size = jh.compress_batch(x[0], quality, restart_interval=case.ri, **how)
    assert one.shape == (case.h, case.w, 1) and np.array_equal(one, g.pixels[0][..., None] / 255) and size == len(g.files['plain'][0])
    image, segments = jh.device_codec(torch.from_numpy(x.copy()).to(dev), quality, 'grey', restart_interval=case.ri, **how)
    assert np.array_equal(image.cpu().numpy(), want) and segments == _segments(g.files['plain'])


# ---- 3. the decoders against the host program -----------------------------------------------------------------------------------------
def _decode(streams, subseq_bits, dev, short=0, expect=0, **bad):
    """nimg_jpeg_grey_decode on streams of one geometry and interval, every output and the workspace between guard bytes ->
    (coef (n, -1), status, rounds) numpy, or the buffers as they were left when the call is expected to be refused."""
    s0, n = streams[0], len(streams)
    blob = b''.join(s.ecd for s in streams)
    ecd = torch.from_numpy(np.frombuffer(blob or b'\0', np.uint8).copy()).to(dev)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s.ecd) for s in streams])]).astype(np.int64)).to(dev)
    huff = torch.from_numpy(np.stack([s.huffman for s in streams])).to(dev)
    lib = _lib().load()
    # `short`: so many bytes less than a batch of no segment bytes needs - the least the library can tell from its arguments
    size = int(lib.nimg_jpeg_grey_decode_workspace_bytes(n, s0.h, s0.w, s0.ri, 0 if short else len(blob), subseq_bits))
    assert size > short
    nb = ops.jpeg_geometry(s0.h, s0.w, *GREY)[0]
    wc, coef = _guarded((n, nb * 64), torch.int16, dev)
    wst, status = _guarded((n,), torch.int32, dev)
    wr, rounds = _guarded((n,), torch.int32, dev)
    ww, ws = _guarded((size - short,), torch.uint8, dev)
    args = dict(n=n, h=s0.h, w=s0.w, ri=s0.ri, sb=subseq_bits, ecd=ecd.data_ptr(), coef=coef.data_ptr())
    args.update(bad)
    rc = lib.nimg_jpeg_grey_decode(args['ecd'], off.data_ptr(), huff.data_ptr(), args['n'], args['h'], args['w'], args['ri'], args['sb'],
                                   args['coef'], status.data_ptr(), rounds.data_ptr(), ws.data_ptr(), size - short, _stream())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert all(_intact(t) for t in (wc, wst, wr, ww)), 'a write outside an output or the workspace'
    if expect:
        assert all(_untouched(t) for t in (wc, wst, wr, ww)), 'a refused call wrote something'
    return coef.cpu().numpy(), status.cpu().numpy(), rounds.cpu().numpy()


def test_status_coefficients_and_rounds_equal_the_host_program(dev):
    """Every golden and damaged stream the sanitized host program has completed cleanly, grouped by geometry and interval so that
    images of different content and damage share a launch; the smallest subsequence length included."""
    streams, results, recoded, hists, done = cases.host_reference()
    assert done.returncode == 0 and done.stderr == b'', done.stderr.decode()[-4000:]
    groups = {}
    for k, s in enumerate(streams):
        groups.setdefault((s.h, s.w, s.ri), []).append(k)
    assert len(streams) > 300 and len(groups) >= 10 and min(cases.SETTINGS[:-1]) == 32
    for key, idx in groups.items():
        part = [streams[k] for k in idx]
        whole = max(max(32, -(-8 * len(s.ecd) // 32) * 32) for s in part)
        for setting in cases.SETTINGS:
            coef, status, rounds = _decode(part, setting or whole, dev)
            for j, k in enumerate(idx):
                r = results[(k, setting)]
                assert status[j] == r.status, (streams[k].name, setting, status[j], r.status)
                assert np.array_equal(coef[j], r.coef), (streams[k].name, setting)
                assert rounds[j] == (r.rounds if setting else 0), (streams[k].name, setting, rounds[j], r.rounds)


def _decode_progressive(files, subseq_bits, dev, short=0, expect=0, rows=None):
    """nimg_jpeg_grey_decode_progressive on files of one geometry, interval and script, between guard bytes."""
    parts = [gref.split(f) for f in files]
    p0, n, ns = parts[0], len(files), len(parts[0]['script'])
    segs = [s for p in parts for s in p['segments']]
    blob = b''.join(segs)
    ecd = torch.from_numpy(np.frombuffer(blob or b'\0', np.uint8).copy()).to(dev)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)).to(dev)
    huff = torch.from_numpy(np.stack([np.stack([gref.table_bytes(t, 3) for t in p['tables']]) for p in parts])).to(dev)
    if rows is None:
        rows = np.array([[1, ss, se, ah, al, lv] for (_, ss, se, ah, al), lv in zip(p0['script'], gref.dpref.levels(p0['script']))], np.int32)
    rows = np.ascontiguousarray(rows, np.int32)
    lib = _lib().load()
    size = int(lib.nimg_jpeg_grey_decode_progressive_workspace_bytes(n, p0['h'], p0['w'], p0['ri'], ns, 0 if short else len(blob), subseq_bits))
    assert size > 0
    nb = ops.jpeg_geometry(p0['h'], p0['w'], *GREY)[0]
    wc, coef = _guarded((n, nb * 64), torch.int16, dev)
    wst, status = _guarded((n,), torch.int32, dev)
    wr, rounds = _guarded((n, ns), torch.int32, dev)
    ww, ws = _guarded((size - short,), torch.uint8, dev)
    rc = lib.nimg_jpeg_grey_decode_progressive(ecd.data_ptr(), off.data_ptr(), rows.ctypes.data, ns, huff.data_ptr(), n, p0['h'], p0['w'],
                                               p0['ri'], subseq_bits, coef.data_ptr(), status.data_ptr(), rounds.data_ptr(), ws.data_ptr(),
                                               size - short, _stream())
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert all(_intact(t) for t in (wc, wst, wr, ww)), 'a write outside an output or the workspace'
    if expect:
        assert all(_untouched(t) for t in (wc, wst, wr, ww)), 'a refused call wrote something'
    return coef.cpu().numpy(), status.cpu().numpy(), rounds.cpu().numpy()


def test_progressive_status_coefficients_and_rounds_equal_the_host_program(dev):
    names, files, results, done = cases.host_progressive_reference()
    assert done.returncode == 0 and done.stderr == b'', done.stderr.decode()[-4000:]
    groups = {}
    for k, f in enumerate(files):
        p = gref.split(f)
        groups.setdefault((p['h'], p['w'], p['ri'], tuple(p['script'])), []).append(k)
    assert len(groups) >= 5 and len(files) >= 30
    for key, idx in groups.items():
        part = [files[k] for k in idx]
        whole = max(max(32, -(-8 * len(s) // 32) * 32) for f in part for s in gref.split(f)['segments'])
        for setting in cases.SETTINGS:
            coef, status, rounds = _decode_progressive(part, setting or whole, dev)
            for j, k in enumerate(idx):
                r = results[(k, setting)]
                assert status[j] == r.status, (names[k], setting, status[j], r.status)
                if r.status == 0:
                    assert np.array_equal(coef[j], r.coef), (names[k], setting)
                assert rounds[j].tolist() == (r.rounds if setting else [0] * len(r.rounds)), (names[k], setting)


# ---- 4. the readers of jpeg_helpers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', cases.CASES, ids=cases.IDS)
def test_decode_batch_equals_pillow(dev, case):
    g = cases.golden()[case.name]
    keys = dict(allow_grey=True, allow_restart=True, allow_progressive=True)
    want = g.pixels[..., None]
    for variant in case.variants:
        for subseq_bits in ((32, 0) if case.h <= 64 else (0,)):
            got = jh.decode_batch(g.files[variant], subseq_bits=subseq_bits, **keys)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (variant, subseq_bits)
        coef, qtables = jh.decode_coefficients(g.files[variant], **keys)
        assert coef.dtype == np.int16 and np.array_equal(coef, np.stack([c.reshape(-1, 64) for c in cases.coefficients(case)])), variant
        assert qtables.shape == (len(want), 1, 64) and np.array_equal(qtables[:, 0], np.repeat(cases.qtable(case)[None], len(want), 0))
    got = jh.decode_batch(g.files[case.variants[0]], as_float=True, device_output=True, **keys)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want.astype(np.float32) / np.float32(255))
    assert np.array_equal(jh.decode_batch(g.files[case.variants[0]][0], **keys), want[:1])          # one file


def test_files_made_here_decode_to_the_pixels_of_their_twins(dev):
    keys = dict(allow_grey=True, allow_progressive=True)
    for tag, (data, case, i) in cases.made_here().items():
        g = cases.golden()[case.name]
        assert np.array_equal(jh.decode_batch(data, **keys)[0], g.pixels[i][..., None]), tag
        assert np.array_equal(jh.decode_coefficients(data, **keys)[0][0], cases.coefficients(case)[i].reshape(-1, 64)), tag
    small = cases.golden()['flat+noise+mixed_20x27_q75_ri0'].files
    base = jh.decode_batch(small['plain'], allow_grey=True)
    for variant in ('prog', 's22', 'opt'):                   # the baseline twin
        assert np.array_equal(jh.decode_batch(small[variant], **keys), base), variant


def test_transcode_batch_equals_the_restatement(dev):
    keys = dict(allow_grey=True, allow_restart=True, allow_progressive=True)
    for name in ('flat+noise+mixed_20x27_q75_ri0', 'noise+mixed_20x27_q75_ri5', 'noise_64x64_q75_ri0', 'noise+mixed_20x27_qt-ones_ri0'):
        case = cases.by_name(name)
        g = cases.golden()[name]
        opt, plain = cases.restated(case, 'opt')[0], cases.restated(case, 'plain')[0]
        for variant in case.variants:                        # jpegtran -optimize of a baseline or a progressive grey-scale file
            again = jh.transcode_batch(g.files[variant], **keys)
            assert again == opt, variant
            assert jh.transcode_batch(g.files[variant], optimize=False, **keys) == plain, variant
            assert np.array_equal(jh.decode_coefficients(again, **keys)[0], jh.decode_coefficients(g.files[variant], **keys)[0])
    data, case, i = cases.made_here()['bands20x27']
    assert jh.transcode_batch([data], **keys) == [cases.restated(case, 'opt')[0][i]]
    with pytest.raises(ValueError, match='grey-scale .one-component. images: progressive=True'):
        jh.transcode_batch(g.files['plain'], progressive=True, **keys)


def test_colour_and_grey_files_mix_in_one_call(dev):
    import jpegrst_cases
    colour = jpegrst_cases.golden()['mixed+noise+smooth_40x56_q75_420_ri5']
    g = cases.golden()
    a, b = g['flat+noise+mixed_20x27_q75_ri0'], g['noise+mixed_20x27_q75_ri5']
    files = [a.files['plain'][1], colour.files['plain'][0], a.files['prog'][2], b.files['opt'][0], colour.files['base'][1], a.files['s22'][0]]
    want = [a.pixels[1][..., None], colour.rgb[0], a.pixels[2][..., None], b.pixels[0][..., None], colour.rgb[1], a.pixels[0][..., None]]
    keys = dict(allow_grey=True, allow_restart=True, allow_progressive=True)
    got = jh.decode_batch(files, **keys)
    assert isinstance(got, list) and len(got) == len(want) and all(np.array_equal(p, q) for p, q in zip(got, want))
    assert [p.shape[-1] for p in got] == [1, 3, 1, 1, 3, 1]
    again = jh.transcode_batch(files, **keys)
    assert all(np.array_equal(p, q) for p, q in zip(jh.decode_batch(again, **keys), want))
    assert [jh.parse_header(f, allow_restart=True, allow_grey=True).ncomp for f in again] == [1, 3, 1, 1, 3, 1]
    with pytest.raises(ValueError, match='decode_coefficients needs files of one geometry'):
        jh.decode_coefficients(files[:2], **keys)
    with pytest.raises(ValueError, match=r'grey-scale file \(3 components needed, the file has 1\)'):
        jh.decode_batch(files, allow_restart=True, allow_progressive=True)
    damaged = files[0][:336] + b'\xff\xd9'                    # eight bytes of data for twelve blocks of noise
    with pytest.raises(ValueError, match=r'damaged JPEG data in file\(s\) \[2\].*(fewer blocks than the scan has|beyond the end of the stream)'):
        jh.decode_batch([files[1], files[3], damaged], **keys)


# ---- 5. every error path, and that a refused call launched nothing ------------------------------------------------------------------------
def test_refused_calls_launch_nothing(dev):
    lib = _lib().load()
    case = cases.by_name('noise+mixed_20x27_q75_ri5')
    n, h, w, ri = 2, 20, 27, 5
    coef, x, qt = _coef(case, dev), _images(case, dev), _qtabs(case, 2, dev)
    need = int(lib.nimg_jpeg_grey_workspace_bytes(n, h, w, ri))
    need_t = int(lib.nimg_jpeg_grey_encode_tables_workspace_bytes(n, h, w, ri))
    tables = torch.from_numpy(np.repeat(gref.ANNEX_K[None], n, 0)).to(dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    def refused(call, expect):
        bufs = {k: _guarded(shape, dtype, dev) for k, (shape, dtype) in dict(
            coef=((n, 12, 64), torch.int16), out=((4096,), torch.uint8), lengths=((n,), torch.int32), status=((n,), torch.int32),
            hist=((n, 2, 257), torch.int32), y=((n, h, w, 1), torch.uint8), ws=((max(need, need_t),), torch.uint8)).items()}
        rc = call({k: v[1].data_ptr() for k, v in bufs.items()})
        torch.cuda.synchronize()
        assert rc == expect, (rc, expect)
        assert all(_untouched(whole) for whole, _ in bufs.values()), 'a refused call wrote something'

    st = _stream()
    # sizes of nothing
    assert lib.nimg_jpeg_grey_workspace_bytes(n, 0, w, ri) == 0 == lib.nimg_jpeg_grey_workspace_bytes(n, h, 4097, ri)
    assert lib.nimg_jpeg_grey_workspace_bytes(n, h, w, 65536) == 0 == lib.nimg_jpeg_grey_encode_tables_workspace_bytes(65536, h, w, 0)
    assert lib.nimg_jpeg_grey_decode_workspace_bytes(n, h, w, -1, 100, 0) == 0 == lib.nimg_jpeg_grey_decode_workspace_bytes(n, h, w, 0, 100, 48)
    assert lib.nimg_jpeg_grey_decode_progressive_workspace_bytes(n, h, w, 0, 65, 100, 0) == 0
    # NIMG_ERR_ARG: null pointers, sizes, qualities and intervals outside their range; NIMG_ERR_WORKSPACE: one byte short
    for quality, hh, xp in ((0, h, x.data_ptr()), (101, h, x.data_ptr()), (75, 0, x.data_ptr()), (75, 4097, x.data_ptr()), (75, h, None)):
        refused(lambda b: lib.nimg_jpeg_grey_transform(xp, 1, n, hh, w, quality, b['coef'], b['ws'], need, st), ERR_ARG)
    refused(lambda b: lib.nimg_jpeg_grey_transform(x.data_ptr(), 1, n, h, w, 75, b['coef'], b['ws'], need - 1, st), ERR_WORKSPACE)
    refused(lambda b: lib.nimg_jpeg_grey_transform(x.data_ptr(), 1, -1, h, w, 75, b['coef'], b['ws'], need, st), ERR_ARG)
    refused(lambda b: lib.nimg_jpeg_grey_transform_tables(x.data_ptr(), 1, n, h, w, None, n, b['coef'], err.data_ptr(), b['ws'], need, st), ERR_ARG)
    refused(lambda b: lib.nimg_jpeg_grey_transform_tables(x.data_ptr(), 1, n, h, w, qt.data_ptr(), n, b['coef'], None, b['ws'], need, st), ERR_ARG)
    refused(lambda b: lib.nimg_jpeg_grey_transform_tables(x.data_ptr(), 1, n, h, w, qt.data_ptr(), n, b['coef'], err.data_ptr(), b['ws'], need - 1,
                                                          st), ERR_WORKSPACE)
    for interval in (-1, 65536):
        refused(lambda b: lib.nimg_jpeg_grey_encode(coef.data_ptr(), n, h, w, interval, b['out'], 4096, b['lengths'], b['ws'], need, st), ERR_ARG)
        refused(lambda b: lib.nimg_jpeg_grey_histogram(coef.data_ptr(), n, h, w, interval, b['hist'], st), ERR_ARG)
        refused(lambda b: lib.nimg_jpeg_grey_encode_tables(coef.data_ptr(), n, h, w, interval, tables.data_ptr(), b['out'], 4096, b['lengths'],
                                                           b['status'], b['ws'], need_t, st), ERR_ARG)
    refused(lambda b: lib.nimg_jpeg_grey_encode(None, n, h, w, ri, b['out'], 4096, b['lengths'], b['ws'], need, st), ERR_ARG)
    refused(lambda b: lib.nimg_jpeg_grey_encode(coef.data_ptr(), n, h, w, ri, b['out'], 4096, b['lengths'], b['ws'], need - 1, st), ERR_WORKSPACE)
    refused(lambda b: lib.nimg_jpeg_grey_histogram(None, n, h, w, ri, b['hist'], st), ERR_ARG)
    refused(lambda b: lib.nimg_jpeg_grey_encode_tables(coef.data_ptr(), n, h, w, ri, None, b['out'], 4096, b['lengths'], b['status'], b['ws'],
                                                       need_t, st), ERR_ARG)
    refused(lambda b: lib.nimg_jpeg_grey_encode_tables(coef.data_ptr(), n, h, w, ri, tables.data_ptr(), b['out'], 4096, b['lengths'], b['status'],
                                                       b['ws'], need_t - 1, st), ERR_WORKSPACE)
    refused(lambda b: lib.nimg_jpeg_grey_reconstruct_tables(coef.data_ptr(), n, h, w, None, b['y'], 1, b['ws'], need, st), ERR_ARG)
    refused(lambda b: lib.nimg_jpeg_grey_reconstruct_tables(coef.data_ptr(), n, h, w, qt.data_ptr(), b['y'], 1, b['ws'], need - 1, st),
            ERR_WORKSPACE)
    # n == 0 is a no-op: success, and nothing is written
    refused(lambda b: lib.nimg_jpeg_grey_transform(None, 1, 0, h, w, 75, b['coef'], b['ws'], 0, st), 0)
    refused(lambda b: lib.nimg_jpeg_grey_encode(None, 0, h, w, ri, b['out'], 4096, b['lengths'], b['ws'], 0, st), 0)
    refused(lambda b: lib.nimg_jpeg_grey_histogram(None, 0, h, w, ri, b['hist'], st), 0)
    refused(lambda b: lib.nimg_jpeg_grey_encode_tables(None, 0, h, w, ri, None, b['out'], 4096, b['lengths'], b['status'], b['ws'], 0, st), 0)
    refused(lambda b: lib.nimg_jpeg_grey_reconstruct_tables(None, 0, h, w, None, b['y'], 1, b['ws'], 0, st), 0)
    refused(lambda b: lib.nimg_jpeg_grey_decode(None, None, None, 0, h, w, ri, 0, b['coef'], b['status'], b['lengths'], b['ws'], 0, st), 0)
    refused(lambda b: lib.nimg_jpeg_grey_decode_progressive(None, None, None, 1, None, 0, h, w, ri, 0, b['coef'], b['status'], b['lengths'],
                                                            b['ws'], 0, st), 0)
    # the decoders: their own guarded calls
    stream = [s for s in cases.valid_streams() if s.name.startswith('noise+mixed_20x27_q75_ri5/plain/')]
    for bad in (dict(sb=48), dict(sb=-32), dict(ri=65536), dict(h=0), dict(w=4097), dict(ecd=None), dict(coef=None), dict(n=-1)):
        _decode(stream, 0, dev, expect=ERR_ARG, **bad)
    for short in (1, 2048):
        _decode(stream, 0, dev, short=short, expect=ERR_WORKSPACE)
    prog = [cases.golden()['flat+noise+mixed_20x27_q75_ri0'].files['prog'][1]]
    rows = np.array([[1, ss, se, ah, al, lv] for (_, ss, se, ah, al), lv in zip(gref.SCRIPT_STD, gref.dpref.levels(gref.SCRIPT_STD))], np.int32)
    for s, c, v in ((0, 0, 7), (0, 0, 2), (1, 0, 4), (3, 3, 1), (5, 4, 1), (2, 2, 62), (4, 5, 1)):          # (scan, column, value)
        bad = rows.copy()
        bad[s, c] = v
        _decode_progressive(prog, 0, dev, expect=ERR_ARG, rows=bad)
    _decode_progressive(prog, 0, dev, short=1, expect=ERR_ARG)


# ---- 6. what stays out says so ----------------------------------------------------------------------------------------------------------
def test_what_is_out_is_refused_by_name(dev):
    x = cases.build(cases.by_name('flat+noise+mixed_20x27_q75_ri0'))[..., None]
    for call in (lambda: jh.encode_batch(x, 75, progressive=True), lambda: jh.compress_batch(x, 75, progressive=True),
                 lambda: jh.device_codec(torch.from_numpy(x.copy()).to(dev), 75, progressive=True)):
        with pytest.raises(ValueError, match='grey-scale .one-component. images: progressive=True'):
            call()
    for name, call in (('rate_distortion', lambda: jh.rate_distortion(x, [50, 75])),
                       ('rate_distortion_tables', lambda: jh.rate_distortion_tables(x, np.ones((1, 2, 64)))),
                       ('match_quality_batch', lambda: jh.match_quality_batch(x)), ('match_quality', lambda: jh.match_quality(x[0]))):
        with pytest.raises(ValueError, match='grey-scale .one-component. images: {} is not supported'.format(name)):
            call()
    for subsampling in ('4:2:0', '4:2:2'):
        with pytest.raises(ValueError, match='takes no chroma sub-sampling'):
            jh.encode_batch(x, 75, subsampling)
        with pytest.raises(ValueError, match='takes no chroma sub-sampling'):
            jh.compress_batch(x[0], 75, subsampling=subsampling)
    with pytest.raises(ValueError, match="subsampling 'grey' needs"):
        jh.encode_batch(np.zeros((1, 8, 8, 3), np.uint8), 75, 'grey')
    xd = torch.from_numpy(x.copy()).to(dev)
    from neural_imaging_amd.models.jpeg import JPEG
    for codec in ('libjpeg', 'soft', 'libjpeg+identity'):      # the models: the real codec, the differentiable one, straight-through
        model = JPEG(75, codec, device=dev)
        with pytest.raises(ValueError, match='the JPEG model takes .n,h,w,3. batches: grey-scale'):
            model.forward(xd.float() / 255)
        with pytest.raises(ValueError, match=r'process_files needs an \(n,h,w,3\) batch'):
            model.process_files(x.astype(np.float32) / 255)
    with pytest.raises(ValueError, match='NHW3'):
        ops.jpeg_ste_shape(xd, 1, 1)
    with pytest.raises(ValueError, match='no chroma to sub-sample'):
        ops.jpeg_transform(xd, 75, 2, 2)
    with pytest.raises(ValueError, match='grey-scale factors with an .n,h,w,3. batch'):
        ops.jpeg_transform(xd.expand(-1, -1, -1, 3).contiguous(), 75, *GREY)
    for bad in (xd.double(), xd.expand(-1, -1, -1, 4).contiguous(), xd.expand(-1, -1, -1, 2).contiguous()):          # the old wording stays
        with pytest.raises(RuntimeError, match=r'jpeg_transform needs an \(n,h,w,3\) float32 or uint8 tensor'):
            ops.jpeg_transform(bad, 75)
    with pytest.raises(RuntimeError, match=r'jpeg_transform_items needs an \(n,h,w,3\) float32 or uint8 tensor'):
        ops.jpeg_transform_items(xd, [75, 75, 75])
    coef = _coef(cases.by_name('flat+noise+mixed_20x27_q75_ri0'), dev)
    with pytest.raises(RuntimeError, match=r'Huffman tables .*\(3, 2, 272\) uint8 needed'):
        ops.jpeg_decode(torch.zeros(8, dtype=torch.uint8, device=dev), torch.zeros(4, dtype=torch.int64, device=dev),
                        torch.zeros((3, 6, 272), dtype=torch.uint8, device=dev), 20, 27, *GREY)
    with pytest.raises(RuntimeError, match=r'tables .*\(3, 1, 64\) 16-bit integers needed'):
        ops.jpeg_reconstruct_tables(coef, 20, 27, torch.ones((3, 3, 64), dtype=torch.int16, device=dev), *GREY)
    with pytest.raises(RuntimeError, match='coefficients .* do not match the geometry'):
        ops.jpeg_encode(coef, 20, 27, 1, 1)                  # 12 blocks are no colour image
