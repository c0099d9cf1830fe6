"""The lossless transforms on the GPU: ops.jpeg_lossless against the sanitized host program (tests/jpegxform_host.cpp)
bit for bit on every job - every operation, sampling, size and crop, stamped tensors of one and of three images, between guard bytes -,
transcode_batch(lossless=) byte for byte against the restatement's files (tests/jpegxform_ref.py; golden/jpeg_lossless.npz) with optimal
and Annex K tables, progressive and with restart intervals, decode_batch of what it wrote against the pixels Pillow decodes from the same
file, decode_coefficients against the restatement, per-file operations in one call with the library calls counted, the algebra on the
device path, and every refusal - of the library with nothing launched, of the Python layer with nothing called.  Everything is exact."""
import ctypes

import numpy as np
import pytest
import torch

import jpegxform_cases as cases
import jpegxform_ref as xr
from neural_imaging_amd import _lib, ops
from neural_imaging_amd.compression import jpeg_helpers as jh

pytestmark = pytest.mark.gpu
FILL, GUARD = 0xa5, 4096
ALLOW = dict(allow_restart=True, allow_progressive=True, allow_grey=True, allow_sampling=True)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    _lib.load()
    return torch.device('cuda', 0)


@pytest.fixture
def calls(monkeypatch):
    """The entry-point names _lib.call is given, in order; the calls go through."""
    names, call = [], _lib.call

    def recorded(name, *args):
        names.append(name)
        return call(name, *args)
    monkeypatch.setattr(_lib, 'call', recorded)
    return names


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(shape, dtype, dev):
    size = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    whole = torch.full((size + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    return whole, whole[GUARD:GUARD + size].view(dtype).view(shape)


def _intact(whole):
    return bool((whole[:GUARD] == FILL).all()) and bool((whole[-GUARD:] == FILL).all())


# ---- the kernel against the host program ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host(dev):
    results, done = cases.host_jobs()
    assert done.returncode == 0 and not done.stderr, done.stderr.decode(errors='replace')[-2000:]
    return results


@pytest.mark.parametrize('sampling', list(cases.SAMPLINGS))
def test_jpeg_lossless_equals_the_host_program(dev, host, sampling):
    hs, vs = cases.factors(sampling)
    served = 0
    for job in (j for j in cases.JOBS if j.sampling == sampling):
        coef = torch.from_numpy(np.array(cases.job_tensor(job))).to(dev)
        if host[job.name] is None:
            with pytest.raises(ValueError, match='nothing is left'):
                ops.jpeg_lossless(coef, job.h, job.w, hs, vs, job.op, job.crop, job.edge)
            continue
        size, want = host[job.name]
        whole, out = _guarded(want.shape, torch.int16, dev)
        got = ops.jpeg_lossless(coef, job.h, job.w, hs, vs, job.op, job.crop, job.edge, out=out)
        assert got[0] is out and got[1:] == size == ops.jpeg_lossless_geometry(job.h, job.w, hs, vs, job.op, job.crop, job.edge), job.name
        assert np.array_equal(out.cpu().numpy(), want), job.name
        assert _intact(whole), job.name
        served += 1
    assert served >= 60
    job = next(j for j in cases.JOBS if j.sampling == sampling and j.n == 3 and j.op == 'rot90' and host[j.name] is not None)
    fresh = ops.jpeg_lossless(torch.from_numpy(np.array(cases.job_tensor(job))).to(dev), job.h, job.w, hs, vs, 'rot90', None, 'trim')
    assert np.array_equal(fresh[0].cpu().numpy(), host[job.name][1])                       # without `out`: a tensor of its own


# ---- transcode_batch against the restatement's files and Pillow's pixels -----------------------------------------------------------------------
def _groups():
    """(operation, crop) -> the file cases that take it and are not refused: one transcode_batch call each."""
    out = {}
    for case in cases.FILE_CASES:
        if cases.expected_size(case) is not None:
            out.setdefault((case.op, case.crop), []).append(case)
    return out


@pytest.fixture(scope='module')
def transcoded(dev):
    """case name -> the file transcode_batch(lossless=, crop=, edge='trim') wrote for it; every (operation, crop) in one call."""
    sources, _ = cases.golden()
    out = {}
    for (op, crop), group in _groups().items():
        files = jh.transcode_batch([sources[c.source.name] for c in group], lossless=op, crop=crop, edge='trim', **ALLOW)
        out.update({c.name: f for c, f in zip(group, files)})
    return out


def test_transcode_batch_equals_the_restatement(dev, transcoded):
    _, made = cases.golden()
    assert len(transcoded) == sum(m is not None for m in made.values()) >= 150
    for name, data in transcoded.items():
        assert data == made[name].data, name


def test_decode_batch_of_the_output_equals_pillow(dev, transcoded):
    _, made = cases.golden()
    names = list(transcoded)
    images = jh.decode_batch([transcoded[n] for n in names], **ALLOW)
    for name, got in zip(names, images):
        m = made[name]
        got = got[..., 0] if got.shape[-1] == 1 else got
        assert got.dtype == np.uint8 and got.shape[:2] == (m.size[1], m.size[0]) and cases.crc(got) == m.crc, name
        assert m.pixels is None or np.array_equal(got, m.pixels), name


def test_decode_coefficients_of_the_output_equal_the_restatement(dev, transcoded):
    sources, _ = cases.golden()
    for s in cases.SOURCES:
        p = xr.parse(sources[s.name])
        for op in ('rot90', 'transverse'):
            name = '{}|{}|trim'.format(s.name, op)
            if name not in transcoded:
                continue
            want, h, w, hs, vs = xr.transform(p['coefs'], p['h'], p['w'], p['hs'], p['vs'], op, None, 'trim')
            coef, qt = jh.decode_coefficients(transcoded[name], **ALLOW)
            assert np.array_equal(coef.reshape(-1), xr.flat(want)) and np.array_equal(qt[0], xr.tables(p['qtables'], op)), name
            hd = jh.parse_header(transcoded[name], **ALLOW)
            assert (hd.h, hd.w) == (h, w) and ((hd.hs, hd.vs) == (hs, vs) or hd.ncomp == 1) and hd.restart_interval == p['ri'], name


VARIANTS = [  # (source, operation, edge, crop): Annex K tables, progressive where the output factors allow it, restart intervals kept
    ('p420_24x40_rst2', 'rot90', 'trim', None), ('p420_24x40_rst2', 'hflip', 'trim', None), ('p422_24x40_prog', 'transpose', 'perfect', None),
    ('w440_24x40', 'transpose', 'perfect', None), ('p420_64x96', 'rot270', 'perfect', (16, 16, 32, 48)), ('grey_33x50_rst3', 'transverse', 'trim', None),
    ('w411_33x50_rst2', 'vflip', 'trim', None), ('p444_33x50_opt', 'none', 'perfect', (8, 16, 17, 9)),
]


@pytest.mark.parametrize('name,op,edge,crop', VARIANTS, ids=['{}-{}'.format(v[0], v[1]) for v in VARIANTS])
def test_optimize_progressive_and_restart_compose(dev, name, op, edge, crop):
    data = cases.golden()[0][name]
    keys = dict(lossless=op, edge=edge, crop=crop, **ALLOW)
    assert jh.transcode_batch(data, **keys) == [xr.transcode(data, op, crop, edge)]
    assert jh.transcode_batch(data, optimize=False, **keys) == [xr.transcode(data, op, crop, edge, optimize=False)]
    s = cases.source_by_name(name)
    hs, vs = xr.size(s.h, s.w, *cases.factors(s.sampling), op, crop, edge)[2:]
    if (hs, vs) in ops.JPEG_SUBSAMPLING.values():
        assert jh.transcode_batch(data, progressive=True, **keys) == [xr.transcode(data, op, crop, edge, progressive=True)]
    else:
        with pytest.raises(ValueError, match='progressive=True'):
            jh.transcode_batch(data, progressive=True, **keys)


def test_a_transposed_file_is_written_without_allow_sampling_and_read_with_it(dev):
    data = cases.golden()[0]['p420_24x40_rst2']
    plain = jh.encode_batch(cases.source_image(cases.source_by_name('p422_24x40_prog')), 50, '4:2:2')
    out = jh.transcode_batch(plain, lossless='rot90')                                           # 4:2:2 in, 4:4:0 out: no keyword needed
    assert out == [xr.transcode(plain[0], 'rot90')]
    with pytest.raises(ValueError, match='unsupported sampling factors'):
        jh.decode_batch(out)
    assert jh.parse_header(out[0], allow_sampling=True)[:4] == (40, 24, 1, 2)
    assert jh.transcode_batch(data, lossless='none', allow_restart=True) == jh.transcode_batch(data, allow_restart=True)


# ---- one call, many files and operations ----------------------------------------------------------------------------------------------------
def test_per_file_operations_in_one_call(dev, calls, transcoded):
    sources, made = cases.golden()
    picks = [('p420_64x96', 'rot90'), ('p420_24x40_rst2', 'none'), ('p420_64x96', 'hflip'), ('grey_8x40', 'transpose'), ('p420_64x96', 'rot90'),
             ('w410_16x32', 'rot270'), ('p420_64x96', 'none'), ('p444_8x8', 'vflip'), ('grey_8x40', 'transpose'), ('p422_24x40_prog', 'transverse')]
    files, names = [sources[s] for s, _ in picks], [op for _, op in picks]
    del calls[:]
    out = jh.transcode_batch(files, lossless=names, edge='trim', **ALLOW)
    taken = list(calls)
    assert out == [made['{}|{}|trim'.format(s, op)].data for s, op in picks]                 # in input order
    # decode groups: 64x96, 24x40 with interval 2, grey 8x40, 4:1:0, 8x8, the progressive 24x40 - and one jpeg_lossless call per group
    # and operation that moves anything: rot90 and hflip of the first, transpose, rot270, vflip, transverse
    assert taken.count('nimg_jpeg_lossless') == 6
    assert sum(n.startswith('nimg_jpeg') and 'decode' in n for n in taken) == 6
    assert taken.count('nimg_jpeg_optimal_tables') == 8                                         # coded per (group, operation)
    del calls[:]
    plain = jh.transcode_batch(files, **ALLOW)
    before = list(calls)
    del calls[:]
    assert jh.transcode_batch(files, lossless='none', **ALLOW) == plain and list(calls) == before and 'nimg_jpeg_lossless' not in before
    del calls[:]
    assert jh.transcode_batch(files, lossless=['none'] * len(files), edge='trim', **ALLOW) == plain and list(calls) == before


# ---- the algebra on the device path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ('p420_16x16', 'p420_64x96', 'grey_8x40', 'w410_16x32', 'w1x4_64x96'))
def test_algebra_on_the_device(dev, name):
    data = cases.golden()[0][name]
    plain = jh.transcode_batch(data, **ALLOW)
    once = jh.transcode_batch([data] * len(xr.OPS), lossless=xr.OPS, **ALLOW)
    assert once[0] == plain[0]
    assert jh.transcode_batch(once, lossless=[xr.INVERSE[op] for op in xr.OPS], **ALLOW) == plain * len(xr.OPS)
    turned = [data]
    for _ in range(4):
        turned = jh.transcode_batch(turned, lossless='rot90', **ALLOW)
    assert turned == plain
    h, w = jh.parse_header(data, **ALLOW)[:2]
    assert jh.transcode_batch(data, crop=(0, 0, w, h), **ALLOW) == plain


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_library_refusals_launch_nothing(dev):
    lib, ARG = _lib.load(), _lib.CONSTANTS['NIMG_ERR_ARG']
    h, w, hs, vs = 33, 50, 2, 2
    nb = ops.jpeg_geometry(h, w, hs, vs)[0]
    coef = torch.zeros((2, nb, 64), dtype=torch.int16, device=dev)
    whole, out = _guarded((2, nb, 64), torch.int16, dev)
    got = (ctypes.c_int * 4)(-7, -7, -7, -7)
    ptrs = [ctypes.byref(got, 4 * k) for k in range(4)]

    def run(n=2, h=h, w=w, hs=hs, vs=vs, nc=3, op=0, crop=(0, 0, 0, 0), trim=0, coef=coef.data_ptr(), out=out.data_ptr(), ptrs=ptrs):
        return lib.nimg_jpeg_lossless(coef, n, h, w, hs, vs, nc, op, *crop, trim, out, *ptrs, _stream())

    refused = [run(op=8), run(op=-1), run(hs=3, vs=1), run(hs=4, vs=4), run(nc=2), run(nc=1), run(nc=1, hs=1, vs=1, n=-1),
               run(crop=(8, 0, 16, 16)), run(crop=(0, 8, 16, 16)), run(crop=(16, 16, 48, 16)), run(crop=(0, 0, 16, 0)), run(crop=(16, 0, 0, 0)),
               run(op=1), run(op=2), run(op=5), run(op=6), run(op=7, trim=0), run(op=4), run(h=9, w=17, op=2, trim=1),
               run(crop=(0, 32, 50, 1), op=2, trim=1), run(coef=None), run(out=None), run(ptrs=[None] + ptrs[1:]), run(ptrs=ptrs[:3] + [None]),
               run(n=0), run(n=65536), run(h=0), run(w=4097)]
    assert set(refused) == {ARG}, refused
    assert lib.nimg_jpeg_lossless_geometry(h, w, hs, vs, 3, 1, 0, 0, 0, 0, 0, *ptrs) == ARG
    assert lib.nimg_jpeg_lossless_geometry(h, w, hs, vs, 3, 0, 0, 0, 0, 0, 0, None, *ptrs[1:]) == ARG
    torch.cuda.synchronize()
    assert bool((whole == FILL).all()) and list(got) == [-7] * 4, 'a refused call wrote'
    assert run(nc=1, hs=1, vs=1, n=0, coef=None, out=None) == 0                              # a grey-scale batch of no images: a no-op
    assert run(op=3) == 0 and list(got) == [50, 33, 2, 2]                                        # and the same arguments, whole, are served
    assert run(op=1, trim=1) == 0 and list(got) == [33, 48, 2, 2]
    assert lib.nimg_jpeg_lossless_geometry(h, w, hs, vs, 3, 6, 16, 16, 20, 17, 1, *ptrs) == 0 and list(got) == [16, 16, 2, 2]
    torch.cuda.synchronize()
    assert _intact(whole)


def test_python_refusals_call_nothing(dev, calls):
    sources, _ = cases.golden()
    ragged, aligned = sources['p444_33x50_opt'], sources['p420_64x96']
    coef = torch.zeros((1, ops.jpeg_geometry(33, 50, 2, 2)[0], 64), dtype=torch.int16, device=dev)
    del calls[:]
    for keys in (dict(lossless='hflip'), dict(lossless='rot90'), dict(lossless=['none', 'rot180']), dict(lossless='rot45'), dict(lossless=['hflip']),
                 dict(lossless='hflip', edge='keep'), dict(crop=(8, 0, 16, 16)), dict(crop=(0, 0, 64, 40)), dict(crop=(0, 0, 16)),
                 dict(lossless='rot180', crop=(0, 32, 48, 1), edge='trim')):
        with pytest.raises(ValueError):
            jh.transcode_batch([aligned, ragged], **dict(ALLOW, **keys))
    with pytest.raises(ValueError, match='progressive=True: progressive files are not written with the sampling factors 1x2'):
        jh.transcode_batch(sources['p422_24x40_prog'], lossless='rot90', edge='trim', progressive=True, **ALLOW)
    for args in ((33, 50, 2, 2, 'vflip'), (33, 50, 2, 2, 'none', (0, 8, 16, 16)), (33, 50, 2, 2, 'flip'), (33, 50, 2, 2, 'hflip', None, 'cut'),
                 (33, 50, 3, 1, 'none')):
        with pytest.raises(ValueError):
            ops.jpeg_lossless(coef, *args)
    with pytest.raises(RuntimeError, match='do not match the geometry'):
        ops.jpeg_lossless(coef, 32, 50, 2, 2, 'none')
    with pytest.raises(RuntimeError, match='jpeg_lossless: output'):
        ops.jpeg_lossless(coef, 33, 50, 2, 2, 'transpose', out=torch.empty_like(coef)[:, :-1])
    assert calls == []
