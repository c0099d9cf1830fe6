"""The samplings 4:4:0, 4:1:1, 4:1:0, 1x4 and 2x4 on the GPU: decode_batch(files, allow_sampling=True) against the
pixels Pillow decodes - byte for byte, every golden file, at scale 1, 2, 4 and 8, as uint8, float and device output -,
decode_coefficients against the restatement, status, coefficients and synchronisation rounds against the sanitized host programs at two
subsequence lengths, baseline and progressive twins, a call that mixes samplings and a grey file, transcode_batch, and the
nimg_jpeg_sampling_* entry points between guard bytes with what they refuse.  Every expectation is exact."""
import ctypes
import io

import numpy as np
import pytest
import torch

import jpegscale_cases as scale_cases
import jpegsamp_cases as cases
import jpegsamp_ref as sr
from neural_imaging_amd import _lib, ops
from neural_imaging_amd.compression import jpeg_helpers as jh

pytestmark = pytest.mark.gpu
FILL, GUARD = 0xa5, 4096
ALLOW = dict(allow_restart=True, allow_progressive=True, allow_sampling=True)
VARIED = [c for c in cases.CASES if (c.h, c.w) == cases.VARIED and c.quality == 90]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    _lib.load()
    return torch.device('cuda', 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(shape, dtype, dev):
    size = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    whole = torch.full((size + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    return whole, whole[GUARD:GUARD + size].view(dtype).view(shape)


def _intact(whole):
    return bool((whole[:GUARD] == FILL).all()) and bool((whole[-GUARD:] == FILL).all())


def _untouched(whole):
    return bool((whole == FILL).all())


def _check_against_golden(case, s, got):
    g = cases.golden()[case.name]
    want = cases.expected(case, s)
    assert got.dtype == np.uint8 and got.shape == want.shape, (case.name, s, got.shape)
    if cases.askable(case, s):
        assert cases.crc(got) == g.crcs[s], (case.name, s)
        if s in g.pixels:
            assert np.array_equal(got, g.pixels[s]), (case.name, s)
    assert np.array_equal(got, want), (case.name, s)


# ---- decode_batch ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def decoded(dev):
    """scale -> the list decode_batch returns for every golden file in one call, computed once."""
    files = [f for _, _, f in cases.golden_files()]
    return {s: jh.decode_batch(files, scale=s, **ALLOW) for s in cases.SCALES}


@pytest.mark.parametrize('s', cases.SCALES)
def test_decode_batch_equals_pillow(decoded, s):
    out = decoded[s]
    assert isinstance(out, list) and len(out) == len(cases.golden_files())
    for (case, _, _), got in zip(cases.golden_files(), out):
        _check_against_golden(case, s, got)


@pytest.mark.parametrize('s', cases.SCALES)
def test_as_float_and_device_output(dev, decoded, s):
    files = [f for _, _, f in cases.golden_files()]
    as_float = jh.decode_batch(files, as_float=True, scale=s, **ALLOW)
    on_device = jh.decode_batch(files, device_output=True, scale=s, **ALLOW)
    on_device_float = jh.decode_batch(files, as_float=True, device_output=True, scale=s, **ALLOW)
    for u8, f32, d8, d32 in zip(decoded[s], as_float, on_device, on_device_float):
        want = u8.astype(np.float32) / np.float32(255)
        assert f32.dtype == np.float32 and f32.shape == u8.shape and np.array_equal(f32.view(np.uint32), want.view(np.uint32))
        assert d8.is_cuda and d8.dtype == torch.uint8 and np.array_equal(d8.cpu().numpy(), u8)
        assert d32.is_cuda and d32.dtype == torch.float32 and np.array_equal(d32.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_without_the_keyword_nothing_changes(dev):
    g = cases.golden()
    for case in VARIED:
        for call in (jh.decode_batch, jh.decode_coefficients, jh.transcode_batch):
            with pytest.raises(ValueError, match=r'unsupported sampling factors .* \(luma 1x1, 2x1 or 2x2 over 1x1 chroma\)'):
                call(g[case.name].files['plain'])


def test_decode_coefficients_equal_the_restatement(dev):
    for case, variant, data in cases.golden_files():
        coef, qt = jh.decode_coefficients(data, **ALLOW)
        assert coef.dtype == np.int16 and coef.shape == (1, ops.jpeg_geometry(case.h, case.w, *cases.factors(case))[0], 64)
        assert np.array_equal(coef.reshape(-1), cases.flat_coefficients(case)), (case.name, variant)
        assert np.array_equal(qt[0], cases.table_words(case))


@pytest.mark.parametrize('case', VARIED, ids=lambda c: c.sampling)
def test_twins_give_equal_coefficients(dev, case):
    files = cases.golden()[case.name].files
    got = {v: jh.decode_coefficients(f, device_output=True, **ALLOW)[0] for v, f in files.items()}
    assert set(got) == set(cases.VARIANTS)
    for v in cases.VARIANTS[1:]:
        assert torch.equal(got[v], got['plain']), v


@pytest.mark.parametrize('s', cases.SCALES)
def test_samplings_and_a_grey_file_in_one_call(dev, s):
    size = (17, 9)
    old = {c.sampling: c for c in scale_cases.CASES if (c.h, c.w) == size}
    new = {c.sampling: c for c in cases.CASES if (c.h, c.w) == (17, 33)}
    picked = [(scale_cases, old['4:2:0']), (cases, new['4:4:0']), (cases, new['4:1:1']), (scale_cases, old['L']), (cases, new['4:1:0'])]
    files = [(m.golden()[0] if m is scale_cases else m.golden())[c.name].files['plain'] for m, c in picked]
    got = jh.decode_batch(files, scale=s, allow_grey=True, allow_sampling=True)
    assert isinstance(got, list) and [y.shape[-1] for y in got] == [3, 3, 3, 1, 3]
    for (m, c), image in zip(picked, got):
        assert np.array_equal(image, m.expected(c, s)), (c.name, s)
    # files of ONE size whose samplings differ are different geometries too: a list, in input order
    same = [new['4:1:1'], new['4:4:0'], new['4:1:1']]
    out = jh.decode_batch([cases.golden()[c.name].files['plain'] for c in same], scale=s, allow_sampling=True)
    assert isinstance(out, list)
    for c, image in zip(same, out):
        _check_against_golden(c, s, image)


# ---- the decoders against the host programs ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_baseline(dev):
    """The sanitized host program's results, built and run once (and shared with test_jpegsamp_host.py in one process)."""
    return cases.host_baseline()


@pytest.fixture(scope='module')
def host_progressive(dev):
    return cases.host_progressive()


def _decode(streams, subseq_bits, dev):
    """nimg_jpeg_sampling_decode on streams of one geometry and interval, every output and the workspace between guard bytes."""
    s0, n = streams[0], len(streams)
    blob = b''.join(s.ecd for s in streams)
    ecd = torch.from_numpy(np.frombuffer(blob or b'\0', np.uint8).copy()).to(dev)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s.ecd) for s in streams])]).astype(np.int64)).to(dev)
    huff = torch.from_numpy(np.stack([s.huffman for s in streams])).to(dev)
    lib = _lib.load()
    size = int(lib.nimg_jpeg_sampling_decode_workspace_bytes(n, s0.h, s0.w, s0.hs, s0.vs, s0.ri, len(blob), subseq_bits))
    assert size > 0
    nb = ops.jpeg_geometry(s0.h, s0.w, s0.hs, s0.vs)[0]
    wc, coef = _guarded((n, nb * 64), torch.int16, dev)
    wst, status = _guarded((n,), torch.int32, dev)
    wr, rounds = _guarded((n,), torch.int32, dev)
    ww, ws = _guarded((size,), torch.uint8, dev)
    rc = lib.nimg_jpeg_sampling_decode(ecd.data_ptr(), off.data_ptr(), huff.data_ptr(), n, s0.h, s0.w, s0.hs, s0.vs, s0.ri, subseq_bits,
                                       coef.data_ptr(), status.data_ptr(), rounds.data_ptr(), ws.data_ptr(), size, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert all(_intact(t) for t in (wc, wst, wr, ww)), 'a write outside an output or the workspace'
    return coef.cpu().numpy(), status.cpu().numpy(), rounds.cpu().numpy()


@pytest.mark.parametrize('sampling', cases.SAMPLINGS, ids=lambda v: v.replace(':', ''))
def test_status_coefficients_and_rounds_equal_the_host_program(dev, host_baseline, sampling):
    """Every golden and damaged baseline stream of the sampling, grouped by geometry and interval so that images of different content
    and damage share a launch; the smallest subsequence length included."""
    streams, results, recoded, done = host_baseline
    assert done.returncode == 0, done.stderr.decode()[-4000:]
    groups = {}
    for k, s in enumerate(streams):
        if (s.hs, s.vs) == sr.WIDE[sampling]:
            groups.setdefault((s.h, s.w, s.ri), []).append(k)
    assert sum(len(v) for v in groups.values()) > 60 and min(cases.SETTINGS) == 32 and len(cases.SETTINGS) == 2
    for key, idx in groups.items():
        part = [streams[k] for k in idx]
        for setting in cases.SETTINGS:
            coef, status, rounds = _decode(part, setting, dev)
            for j, k in enumerate(idx):
                r = results[(k, setting)]
                assert status[j] == r.status, (streams[k].name, setting, status[j], r.status)
                assert np.array_equal(coef[j], r.coef), (streams[k].name, setting)
                assert rounds[j] == r.rounds, (streams[k].name, setting, rounds[j], r.rounds)


@pytest.mark.parametrize('sampling', cases.SAMPLINGS, ids=lambda v: v.replace(':', ''))
def test_progressive_status_coefficients_and_rounds_equal_the_host_program(dev, host_progressive, sampling):
    files, results, done = host_progressive
    assert results is not None and done.returncode == 0, done.stderr.decode()[-4000:]
    mine = [(f, r) for f, r in zip(files, results) if (f.hs, f.vs) == sr.WIDE[sampling]]
    assert len(mine) > 20
    for f, r in mine:
        assert r.legal
        ecd = torch.from_numpy(np.frombuffer(b''.join(f.segments) or b'\0', np.uint8).copy()).to(dev)
        off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in f.segments])]).astype(np.int64)).to(dev)
        huff = torch.from_numpy(np.stack(f.tables)[None]).to(dev)
        for setting in cases.SETTINGS:
            coef, status, rounds = ops.jpeg_decode_progressive(ecd, off, huff, cases.dpc.dpref_rows(f.script), f.h, f.w, f.hs, f.vs,
                                                               subseq_bits=setting, restart_interval=f.ri)
            assert int(status[0]) == r.status[setting], (f.name, setting)
            assert np.array_equal(coef.cpu().numpy().reshape(-1), r.coef[setting]), (f.name, setting)
            assert rounds.cpu().numpy()[0].tolist() == r.rounds[setting], (f.name, setting)


# ---- transcode_batch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', VARIED, ids=lambda c: c.sampling)
def test_transcode_batch(dev, case):
    Image = pytest.importorskip('PIL.Image')
    files = cases.golden()[case.name].files
    names = list(files)
    for optimize in (True, False):
        out = jh.transcode_batch([files[v] for v in names], optimize=optimize, **ALLOW)
        for v, data in zip(names, out):
            hd = jh.parse_header(data, **ALLOW)
            assert (hd.h, hd.w, hd.hs, hd.vs) == (case.h, case.w) + cases.factors(case) and not hd.scans, v
            assert hd.restart_interval == cases.restart_interval(case, v) and np.array_equal(hd.qtables, cases.table_words(case))
            coef = jh.decode_coefficients(data, **ALLOW)[0]
            assert np.array_equal(coef.reshape(-1), cases.flat_coefficients(case)), (v, optimize)
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), cases.expected(case, 1)), (v, optimize)
            twin = {0: 'opt' if optimize else 'plain', 1: None if optimize else 'rst1', cases.RSTN: None if optimize else 'rstn'}.get(hd.restart_interval)
            if twin:                                                  # the test writer's file of the same tables and interval
                assert data == files[twin], (v, optimize)
    with pytest.raises(ValueError, match='progressive=True: progressive files are not written with the sampling factors {}x{}'.format(
            *cases.factors(case))):
        jh.transcode_batch(files['plain'], progressive=True, allow_sampling=True)


# ---- the entry points ---------------------------------------------------------------------------------------------------------------
def _tensors(job_cases, dev):
    coef = torch.from_numpy(np.stack([cases.flat_coefficients(c).reshape(-1, 64) for c in job_cases])).to(dev)
    qt = torch.from_numpy(np.stack([cases.table_words(c) for c in job_cases]).view(np.int16)).to(dev)
    return coef, qt


@pytest.mark.parametrize('case', VARIED, ids=lambda c: c.sampling)
def test_reconstruct_and_writer_entries_between_guard_bytes(dev, case):
    twin = next(c for c in cases.CASES if (c.h, c.w, c.sampling) == (case.h, case.w, case.sampling) and c is not case)
    batch = [case, twin, case]
    n, h, w, (hs, vs) = 3, case.h, case.w, cases.factors(case)
    coef, qt = _tensors(batch, dev)
    lib = _lib.load()
    for s in cases.SCALES:
        need = int(lib.nimg_jpeg_sampling_reconstruct_scaled_workspace_bytes(n, h, w, hs, vs, s))
        assert need > 0 and need % 256 == 0
        for u8 in (True, False):
            rows, cols = -(-h // s), -(-w // s)
            wy, y = _guarded((n, rows, cols, 3), torch.uint8 if u8 else torch.float32, dev)
            ww, ws = _guarded((need,), torch.uint8, dev)
            got = ops.jpeg_reconstruct_scaled(coef, h, w, qt, s, hs, vs, out_u8=u8, workspace=ws, out=y)
            want = np.stack([cases.expected(c, s) for c in batch])
            assert got.data_ptr() == y.data_ptr()
            assert np.array_equal(got.cpu().numpy(), want if u8 else want.astype(np.float32) / np.float32(255)), (s, u8)
            assert _intact(wy) and _intact(ww)
            if s == 1:
                wy, y = _guarded((n, h, w, 3), torch.uint8 if u8 else torch.float32, dev)
                ops.jpeg_reconstruct_tables(coef, h, w, qt, hs, vs, out_u8=u8, workspace=ws, out=y)
                assert np.array_equal(y.cpu().numpy(), want if u8 else want.astype(np.float32) / np.float32(255)) and _intact(wy) and _intact(ww)
    for ri in (0, 1, cases.RSTN):
        wh, hist = _guarded((n, 4, 257), torch.int32, dev)
        ops.jpeg_histogram(coef, h, w, hs, vs, out=hist, restart_interval=ri)
        want = np.stack([cases.rref.histograms(cases.coefficients(c), h, w, hs, vs, ri) for c in batch])
        assert np.array_equal(hist.cpu().numpy().view(np.uint32), want) and _intact(wh)
        tables, status = ops.jpeg_optimal_tables(hist)
        assert not status.cpu().numpy().any()
        need_t = int(lib.nimg_jpeg_sampling_encode_tables_workspace_bytes(n, h, w, hs, vs, ri))
        assert need_t > 0
        wt, ws = _guarded((need_t,), torch.uint8, dev)
        wo, out = _guarded((n * ops.jpeg_ecd_bound_tables(h, w, hs, vs, ri),), torch.uint8, dev)
        data, lengths, status = ops.jpeg_encode_tables(coef, tables, h, w, hs, vs, out=out, workspace=ws, restart_interval=ri)
        assert not status.cpu().numpy().any() and _intact(wt) and _intact(wo)
        ends = np.concatenate([[0], np.cumsum(lengths.cpu().numpy())])
        blob = data.cpu().numpy()
        for j, c in enumerate(batch):
            want_file = sr.write_baseline(cases.coefficients(c), h, w, c.quality, hs, vs, ri, optimize=True)
            assert blob[ends[j]:ends[j + 1]].tobytes() == cases.stream_of('', want_file).ecd, (c.name, ri)


def test_the_new_reconstruct_entry_serves_the_three_with_the_bits_of_its_namesake(dev):
    for sampling in ('4:4:4', '4:2:2', '4:2:0'):
        five = scale_cases.batch_of_five(sampling)
        coef = torch.from_numpy(np.stack([scale_cases.flat_coefficients(c).reshape(-1, 64) for c in five])).to(dev)
        qt = torch.from_numpy(np.stack([scale_cases.table_words(c) for c in five]).view(np.int16)).to(dev)
        hs, vs = scale_cases.factors(five[0])
        n, h, w = len(five), five[0].h, five[0].w
        lib = _lib.load()
        for s in cases.SCALES:
            need = int(lib.nimg_jpeg_sampling_reconstruct_scaled_workspace_bytes(n, h, w, hs, vs, s))
            assert need == int(lib.nimg_jpeg_reconstruct_scaled_workspace_bytes(n, h, w, hs, vs, s)) > 0
            want = ops.jpeg_reconstruct_scaled(coef, h, w, qt, s, hs, vs, out_u8=True)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            y = torch.full(tuple(want.shape), FILL, dtype=torch.uint8, device=dev)
            rc = lib.nimg_jpeg_sampling_reconstruct_scaled(coef.data_ptr(), n, h, w, hs, vs, qt.data_ptr(), s, y.data_ptr(), 1, ws.data_ptr(),
                                                           need, _stream())
            assert rc == 0 and torch.equal(y, want), (sampling, s)
        want = ops.jpeg_reconstruct_tables(coef, h, w, qt, hs, vs, out_u8=False)
        y = torch.full(tuple(want.shape), float('nan'), dtype=torch.float32, device=dev)
        need = ops.jpeg_workspace_bytes(n, h, w, hs, vs)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        rc = lib.nimg_jpeg_sampling_reconstruct_tables(coef.data_ptr(), n, h, w, hs, vs, qt.data_ptr(), y.data_ptr(), 0, ws.data_ptr(), need,
                                                       _stream())
        assert rc == 0 and np.array_equal(y.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32)), sampling


def test_refusals_launch_nothing(dev):
    case = next(c for c in cases.CASES if (c.h, c.w, c.sampling) == (17, 33, '4:1:1'))
    coef, qt = _tensors([case], dev)
    h, w, (hs, vs) = case.h, case.w, cases.factors(case)
    lib = _lib.load()
    ARG, WORKSPACE = _lib.CONSTANTS['NIMG_ERR_ARG'], _lib.CONSTANTS['NIMG_ERR_WORKSPACE']
    stream = cases.stream_of('', cases.golden()[case.name].files['plain'])
    ecd = torch.from_numpy(np.frombuffer(stream.ecd, np.uint8).copy()).to(dev)
    off = torch.tensor([0, len(stream.ecd)], dtype=torch.int64, device=dev)
    huff = torch.from_numpy(stream.huffman[None]).to(dev)
    prog = cases.dpc._file('', sr.write_progressive(cases.coefficients(case), h, w, case.quality, hs, vs, cases.dprog.STANDARD), None)
    pecd = torch.from_numpy(np.frombuffer(b''.join(prog.segments), np.uint8).copy()).to(dev)
    poff = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in prog.segments])]).astype(np.int64)).to(dev)
    phuff = torch.from_numpy(np.stack(prog.tables)[None]).to(dev)
    rows = np.ascontiguousarray(cases.dpc.dpref_rows(prog.script), np.int32)
    tables = torch.from_numpy(np.ascontiguousarray(cases.rref.oref.ANNEX_K[None])).to(dev)
    need = {'decode': int(lib.nimg_jpeg_sampling_decode_workspace_bytes(1, h, w, hs, vs, 0, len(stream.ecd), 0)),
            'prog': int(lib.nimg_jpeg_sampling_decode_progressive_workspace_bytes(1, h, w, hs, vs, 0, len(rows), pecd.numel(), 0)),
            'rec': int(lib.nimg_jpeg_sampling_reconstruct_scaled_workspace_bytes(1, h, w, hs, vs, 1)),
            'rec2': int(lib.nimg_jpeg_sampling_reconstruct_scaled_workspace_bytes(1, h, w, hs, vs, 2)),
            'enc': int(lib.nimg_jpeg_sampling_encode_tables_workspace_bytes(1, h, w, hs, vs, 0))}
    # the least the decoders can tell from their arguments: a workspace shorter than a batch of no segment bytes needs
    none = {'decode': int(lib.nimg_jpeg_sampling_decode_workspace_bytes(1, h, w, hs, vs, 0, 0, 0)),
            'prog': int(lib.nimg_jpeg_sampling_decode_progressive_workspace_bytes(1, h, w, hs, vs, 0, len(rows), 0, 0))}
    assert all(v > 0 for v in need.values()) and all(0 < none[k] <= need[k] for k in none)
    big = max(need.values())
    bufs = {k: torch.full(shape, FILL, dtype=torch.uint8, device=dev)
            for k, shape in (('coef', (coef.numel() * 2,)), ('status', (4,)), ('rounds', (4 * len(rows),)), ('y', (h * w * 3,)),
                             ('hist', (4 * 257 * 4,)), ('out', (65536,)), ('lengths', (4,)), ('ws', (big,)))}
    p = {k: v.data_ptr() for k, v in bufs.items()}
    st = _stream()

    def calls(a, b, short):
        """Every new entry with the factors (a, b); short: so many bytes less workspace than it needs."""
        out = {
            'decode': lib.nimg_jpeg_sampling_decode(ecd.data_ptr(), off.data_ptr(), huff.data_ptr(), 1, h, w, a, b, 0, 0, p['coef'], p['status'],
                                                    p['rounds'], p['ws'], (none if short else need)['decode'] - short, st),
            'prog': lib.nimg_jpeg_sampling_decode_progressive(pecd.data_ptr(), poff.data_ptr(), rows.ctypes.data, len(rows), phuff.data_ptr(), 1,
                                                              h, w, a, b, 0, 0, p['coef'], p['status'], p['rounds'], p['ws'],
                                                              (none if short else need)['prog'] - short, st),
            'rec': lib.nimg_jpeg_sampling_reconstruct_tables(coef.data_ptr(), 1, h, w, a, b, qt.data_ptr(), p['y'], 1, p['ws'],
                                                             need['rec'] - short, st),
            'rec2': lib.nimg_jpeg_sampling_reconstruct_scaled(coef.data_ptr(), 1, h, w, a, b, qt.data_ptr(), 2, p['y'], 1, p['ws'],
                                                              need['rec2'] - short, st),
            'enc': lib.nimg_jpeg_sampling_encode_tables(coef.data_ptr(), 1, h, w, a, b, 0, tables.data_ptr(), p['out'], 65536, p['lengths'],
                                                        p['status'], p['ws'], need['enc'] - short, st)}
        if not short:                                                   # (the histogram has no workspace to be short of)
            out['hist'] = lib.nimg_jpeg_sampling_histogram(coef.data_ptr(), 1, h, w, a, b, 0, p['hist'], st)
        return out

    for a, b in ((3, 1), (4, 4), (1, 3), (0, 1), (8, 1)):
        assert set(calls(a, b, 0).values()) == {ARG}, (a, b)
        assert lib.nimg_jpeg_sampling_decode_workspace_bytes(1, h, w, a, b, 0, 100, 0) == 0
        assert lib.nimg_jpeg_sampling_decode_progressive_workspace_bytes(1, h, w, a, b, 0, 10, 100, 0) == 0
        assert lib.nimg_jpeg_sampling_reconstruct_scaled_workspace_bytes(1, h, w, a, b, 2) == 0
        assert lib.nimg_jpeg_sampling_encode_tables_workspace_bytes(1, h, w, a, b, 0) == 0
    short = calls(hs, vs, 1)
    # the progressive launcher has always answered a workspace too short for a batch of no bytes with NIMG_ERR_ARG
    assert short.pop('prog') in (ARG, WORKSPACE) and set(short.values()) == {WORKSPACE}, short
    torch.cuda.synchronize()
    assert all(_untouched(v) for v in bufs.values()), 'a refused call wrote'
    # the entry points of before still refuse the five
    for a, b in sr.WIDE.values():
        assert lib.nimg_jpeg_decode_restart_workspace_bytes(1, h, w, a, b, 0, 100, 0) == 0 == lib.nimg_jpeg_workspace_bytes(1, h, w, a, b)
        assert lib.nimg_jpeg_reconstruct_tables(coef.data_ptr(), 1, h, w, a, b, qt.data_ptr(), p['y'], 1, p['ws'], big, st) == ARG
        assert lib.nimg_jpeg_histogram_restart(coef.data_ptr(), 1, h, w, a, b, 0, p['hist'], st) == ARG
    good = calls(hs, vs, 0)
    torch.cuda.synchronize()
    assert set(good.values()) == {0}, good                               # and the same arguments, whole, are served
