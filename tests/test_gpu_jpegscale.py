"""Scaled JPEG decoding on the GPU: decode_batch(files, scale=s) against the pixels Pillow decodes after
Image.draft() - byte for byte, every golden case, s in 1, 2, 4, 8 -, as_float and device_output, baseline, progressive and restart files
in one batch, colour next to grey, ops.jpeg_reconstruct_scaled against the sanitized host program over csrc/jpegscale.h, scale 1
against jpeg_reconstruct_tables, the library calls decode_batch makes, guard bytes around output and workspace, and what the entry
points refuse.  Every expectation is exact."""
import numpy as np
import pytest
import torch

import jpegscale_cases as cases
from neural_imaging_amd import _lib, ops
from neural_imaging_amd.compression import jpeg_helpers as jh

pytestmark = pytest.mark.gpu
FILL = 0xa5
ALLOW = dict(allow_restart=True, allow_progressive=True, allow_grey=True)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    _lib.load()
    return torch.device('cuda', 0)


def _all_files():
    """[(case, variant, file)] of the golden file, in case order."""
    g = cases.golden()[0]
    return [(c, v, g[c.name].files[v]) for c in cases.CASES for v in c.variants]


def _check_against_golden(case, s, got):
    """`got` against Pillow's pixels, or their CRC32 where the golden file holds no more; against the restatement where Pillow cannot
    be asked."""
    g = cases.golden()[0].get(case.name)                    # None: one of the tiny cases, which the golden file does not hold
    want = cases.expected(case, s)
    assert got.dtype == np.uint8 and got.shape == want.shape, (case.name, s, got.shape)
    if g is not None and cases.askable(case, s):
        assert cases.crc(got) == g.crcs[s], (case.name, s)
        if s in g.pixels:
            assert np.array_equal(got, g.pixels[s]), (case.name, s)
    assert np.array_equal(got, want), (case.name, s)


# ---- decode_batch ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def decoded(dev):
    """scale -> the list decode_batch returns for every golden file in one call, computed once."""
    files = [f for _, _, f in _all_files()]
    return {s: jh.decode_batch(files, scale=s, **ALLOW) for s in cases.SCALES}


@pytest.mark.parametrize('s', cases.SCALES)
def test_decode_batch_equals_pillow(decoded, s):
    out = decoded[s]
    assert isinstance(out, list) and len(out) == len(_all_files())
    for (case, variant, _), got in zip(_all_files(), out):
        _check_against_golden(case, s, got)


@pytest.mark.parametrize('s', cases.SCALES)
def test_decode_batch_of_sizes_pillow_cannot_be_asked_for(dev, s):
    for case in cases.TINY:
        got = jh.decode_batch(cases.restated_file(case), scale=s, allow_grey=True)
        assert got.shape[0] == 1
        _check_against_golden(case, s, got[0])


@pytest.mark.parametrize('s', cases.SCALES)
def test_as_float_and_device_output(dev, decoded, s):
    files = [f for _, _, f in _all_files()]
    as_float = jh.decode_batch(files, as_float=True, scale=s, **ALLOW)
    on_device = jh.decode_batch(files, device_output=True, scale=s, **ALLOW)
    on_device_float = jh.decode_batch(files, as_float=True, device_output=True, scale=s, **ALLOW)
    for u8, f32, d8, d32 in zip(decoded[s], as_float, on_device, on_device_float):
        want = u8.astype(np.float32) / np.float32(255)
        assert f32.dtype == np.float32 and f32.shape == u8.shape and np.array_equal(f32.view(np.uint32), want.view(np.uint32))
        assert d8.is_cuda and d8.dtype == torch.uint8 and np.array_equal(d8.cpu().numpy(), u8)
        assert d32.is_cuda and d32.dtype == torch.float32 and np.array_equal(d32.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('s', cases.SCALES)
@pytest.mark.parametrize('sampling', cases.SAMPLINGS, ids=lambda v: v.replace(':', ''))
def test_baseline_progressive_and_restart_files_make_one_batch(dev, sampling, s):
    case = next(c for c in cases.CASES if (c.h, c.w) == cases.VARIED and c.sampling == sampling)
    g = cases.golden()[0][case.name]
    # the baseline file twice: the two share a group, the progressive and the restart file take one each - still one geometry
    files = [g.files['plain'], g.files['prog'], g.files['rst'], g.files['plain']]
    got = jh.decode_batch(files, scale=s, **ALLOW)
    if s == 1:                                                            # as before this keyword: a list of the same images
        assert isinstance(got, list) and len(got) == 4
    else:
        assert isinstance(got, np.ndarray) and got.shape[0] == 4
        on_device = jh.decode_batch(files, scale=s, device_output=True, **ALLOW)
        assert torch.is_tensor(on_device) and np.array_equal(on_device.cpu().numpy(), got)
    for image in got:
        _check_against_golden(case, s, image)
    # input order: a file of another quality between two groups of the first geometry's files
    other = next(c for c in cases.CASES if (c.h, c.w) == cases.FULL and c.sampling == sampling)
    mixed = jh.decode_batch([g.files['rst'], cases.golden()[0][other.name].files['plain'], g.files['plain']], scale=s, **ALLOW)
    assert isinstance(mixed, list)
    for c, image in zip((case, other, case), mixed):
        _check_against_golden(c, s, image)


@pytest.mark.parametrize('s', cases.SCALES)
def test_colour_and_grey_files_in_one_call(dev, s):
    picked = [c for c in cases.CASES if (c.h, c.w) == (17, 9)]
    assert {c.sampling for c in picked} == set(cases.SAMPLINGS)
    got = jh.decode_batch([cases.golden()[0][c.name].files['plain'] for c in picked], scale=s, allow_grey=True)
    assert isinstance(got, list) and [y.shape[-1] for y in got] == [1 if c.sampling == 'L' else 3 for c in picked]
    for case, image in zip(picked, got):
        _check_against_golden(case, s, image)
    with pytest.raises(ValueError):                                      # the grey file is still refused unless asked for
        jh.decode_batch([cases.golden()[0][c.name].files['plain'] for c in picked], scale=s)


# ---- ops.jpeg_reconstruct_scaled ---------------------------------------------------------------------------------------------------
def _tensors(job_cases, dev):
    """(coefficients (n, real blocks, 64) int16, tables (n, nc, 64) int16 bit patterns, (hs, vs) as the ops take them)."""
    coef = torch.from_numpy(np.stack([cases.flat_coefficients(c).reshape(-1, 64) for c in job_cases])).to(dev)
    qt = torch.from_numpy(np.stack([cases.table_words(c) for c in job_cases]).view(np.int16)).to(dev)
    c0 = job_cases[0]
    return coef, qt, (ops.JPEG_GREY if c0.sampling == 'L' else cases.factors(c0))


def test_reconstruct_scaled_equals_host_program(dev):
    images, done = cases.host_reference()
    assert done.returncode == 0 and done.stderr == b''
    assert any(len(job.cases) == 5 for job in images)
    for job, want in images.items():
        coef, qt, (hs, vs) = _tensors(job.cases, dev)
        c0 = job.cases[0]
        got = ops.jpeg_reconstruct_scaled(coef, c0.h, c0.w, qt, job.scale, hs, vs, out_u8=True)
        assert np.array_equal(got.cpu().numpy(), want), ([c.name for c in job.cases], job.scale)


@pytest.mark.parametrize('sampling', cases.SAMPLINGS, ids=lambda v: v.replace(':', ''))
def test_scale_one_is_reconstruct_tables(dev, sampling):
    for job_cases in (cases.batch_of_five(sampling), [c for c in cases.CASES if c.sampling == sampling and (c.h, c.w) == (37, 53)]):
        coef, qt, (hs, vs) = _tensors(job_cases, dev)
        c0 = job_cases[0]
        for u8 in (True, False):
            want = ops.jpeg_reconstruct_tables(coef, c0.h, c0.w, qt, hs, vs, out_u8=u8)
            got = ops.jpeg_reconstruct_scaled(coef, c0.h, c0.w, qt, 1, hs, vs, out_u8=u8)
            assert got.dtype == want.dtype and got.shape == want.shape
            assert np.array_equal(got.cpu().numpy().view(np.uint8), want.cpu().numpy().view(np.uint8))
        size, factors = ops._jpeg_entry('nimg_jpeg_reconstruct_scaled_workspace_bytes', hs, vs)
        assert getattr(_lib.load(), size)(len(job_cases), c0.h, c0.w, *factors, 1) == ops.jpeg_workspace_bytes(len(job_cases), c0.h, c0.w, hs, vs)


# ---- the library calls --------------------------------------------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    """The entry-point names _lib.call is given, in order; the calls go through."""
    names, call = [], _lib.call

    def recorded(name, *args):
        names.append(name)
        return call(name, *args)
    monkeypatch.setattr(_lib, 'call', recorded)
    return names


def _taken(names):
    out = list(names)
    del names[:]
    return out


def test_library_calls(dev, calls):
    colour = next(c for c in cases.CASES if (c.h, c.w) == cases.VARIED and c.sampling == '4:2:0')
    grey = next(c for c in cases.CASES if (c.h, c.w) == cases.VARIED and c.sampling == 'L')
    g = cases.golden()[0]
    today = {'plain': ['nimg_jpeg_decode_restart', 'nimg_jpeg_reconstruct_tables'],
             'rst': ['nimg_jpeg_decode_restart', 'nimg_jpeg_reconstruct_tables'],
             'prog': ['nimg_jpeg_decode_progressive', 'nimg_jpeg_reconstruct_tables']}
    for variant, want in today.items():
        for case, names in ((colour, want), (grey, [n.replace('nimg_jpeg_', 'nimg_jpeg_grey_').replace('_restart', '') for n in want])):
            data = g[case.name].files[variant]
            jh.decode_batch(data, **ALLOW)
            assert _taken(calls) == names                                  # without the keyword: today's calls
            jh.decode_batch(data, scale=1, **ALLOW)
            assert _taken(calls) == names                                  # scale 1: the same
            for s in cases.REDUCED:
                jh.decode_batch(data, scale=s, **ALLOW)
                scaled = 'nimg_jpeg_reconstruct_scaled_grey' if case is grey else 'nimg_jpeg_reconstruct_scaled'
                assert _taken(calls) == [names[0], scaled]


# ---- guard bytes and refusals ---------------------------------------------------------------------------------------------------------
def _guarded(dev, nbytes, guard=4096):
    """A uint8 device buffer of FILL with `nbytes` in its middle, 256-byte aligned: (the whole buffer, the middle)."""
    whole = torch.full((2 * guard + nbytes,), FILL, dtype=torch.uint8, device=dev)
    return whole, whole[guard:guard + nbytes]


def _guards_intact(whole, nbytes, guard=4096):
    host = whole.cpu().numpy()
    return bool((host[:guard] == FILL).all() and (host[guard + nbytes:] == FILL).all())


@pytest.mark.parametrize('u8', (True, False), ids=('u8', 'f32'))
@pytest.mark.parametrize('s', cases.REDUCED)
@pytest.mark.parametrize('sampling', cases.SAMPLINGS, ids=lambda v: v.replace(':', ''))
def test_guard_bytes(dev, sampling, s, u8):
    five = cases.batch_of_five(sampling)
    coef, qt, (hs, vs) = _tensors(five, dev)
    c0, n, nc = five[0], len(five), 1 if sampling == 'L' else 3
    rows, cols = jh.scaled_size(c0.h, c0.w, s)
    size, factors = ops._jpeg_entry('nimg_jpeg_reconstruct_scaled_workspace_bytes', hs, vs)
    need = int(getattr(_lib.load(), size)(n, c0.h, c0.w, *factors, s))
    assert need > 0 and need % 256 == 0
    out_bytes = n * rows * cols * nc * (1 if u8 else 4)
    whole_y, y = _guarded(dev, out_bytes)
    whole_ws, ws = _guarded(dev, need)
    y = (y if u8 else y.view(torch.float32)).view(n, rows, cols, nc)
    got = ops.jpeg_reconstruct_scaled(coef, c0.h, c0.w, qt, s, hs, vs, out_u8=u8, workspace=ws, out=y)
    want = np.stack([cases.expected(c, s) for c in five])
    assert got.data_ptr() == y.data_ptr()
    assert np.array_equal(got.cpu().numpy(), want if u8 else want.astype(np.float32) / np.float32(255))
    assert _guards_intact(whole_y, out_bytes) and _guards_intact(whole_ws, need)


@pytest.mark.parametrize('grey', (False, True), ids=('colour', 'grey'))
def test_refusals_launch_nothing(dev, grey):
    case = next(c for c in cases.CASES if (c.h, c.w) == (16, 16) and c.sampling == ('L' if grey else '4:2:2'))
    coef, qt, (hs, vs) = _tensors([case], dev)
    lib = _lib.load()
    entry, factors = ops._jpeg_entry('nimg_jpeg_reconstruct_scaled', hs, vs)
    size = entry + '_workspace_bytes'
    need = int(getattr(lib, size)(1, 16, 16, *factors, 2))
    y = torch.full((1, 8, 8, 1 if grey else 3), FILL, dtype=torch.uint8, device=dev)
    ws = torch.full((need,), FILL, dtype=torch.uint8, device=dev)
    ARG, WORKSPACE = _lib.CONSTANTS['NIMG_ERR_ARG'], _lib.CONSTANTS['NIMG_ERR_WORKSPACE']

    def call(coef_p, qt_p, scale, y_p, ws_p, ws_bytes):
        return getattr(lib, entry)(coef_p, 1, 16, 16, *factors, qt_p, scale, y_p, 1, ws_p, ws_bytes, ops._stream())

    good = (coef.data_ptr(), qt.data_ptr(), 2, y.data_ptr(), ws.data_ptr(), need)
    for scale in (0, 3, 5, 16, -2):
        assert call(*good[:2], scale, *good[3:]) == ARG
        assert getattr(lib, size)(1, 16, 16, *factors, scale) == 0
    for k in (0, 1, 3, 4):
        assert call(*[None if j == k else v for j, v in enumerate(good)]) == ARG
    assert call(*good[:5], need - 1) == WORKSPACE and call(*good[:5], 0) == WORKSPACE
    torch.cuda.synchronize()
    assert bool((y == FILL).all()) and bool((ws == FILL).all()), 'a refused call wrote'
    assert call(*good) == 0                                               # and the same arguments, whole, are served
    assert np.array_equal(y.cpu().numpy()[0], cases.expected(case, 2))
    with pytest.raises(RuntimeError, match='workspace of {} bytes, {} needed'.format(need - 1, need)):
        ops.jpeg_reconstruct_scaled(coef, 16, 16, qt, 2, hs, vs, out_u8=True, workspace=ws[:need - 1])
    with pytest.raises(RuntimeError, match='jpeg_reconstruct_scaled: output'):
        ops.jpeg_reconstruct_scaled(coef, 16, 16, qt, 2, hs, vs, out_u8=True, out=torch.empty((1, 16, 16, y.shape[3]), dtype=torch.uint8, device=dev))
