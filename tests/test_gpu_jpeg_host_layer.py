"""The Python layer above the JPEG codec kernels (ops.py's JPEG section, compression/jpeg_helpers.py's writer): what the byte-exact
tests of the files cannot see.
  (a) the library calls a batch costs: one encode per batch, a second one only when the first-guess capacity was short;
  (b) the refusals of the checks every op shares - coefficients, RGB input, workspace -, through every public op that uses them.
Every refusal is raised on the host, before anything is launched."""
import numpy as np
import pytest
import torch

import jpeg_cases
from neural_imaging_amd import _lib, ops
from neural_imaging_amd.compression import jpeg_helpers as jh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    _lib.load()
    return torch.device('cuda', 0)


# ---- (a) the call sequence ----------------------------------------------------------------------------------------------------------
# mode -> (its keyword, the ops.* bound its first-guess capacity is cut by, the calls behind the transform)
MODES = {
    'plain': ({}, 'jpeg_ecd_bound', ['nimg_jpeg_encode_restart']),
    'optimize': ({'optimize': True}, 'jpeg_ecd_bound_tables',
                 ['nimg_jpeg_histogram_restart', 'nimg_jpeg_optimal_tables', 'nimg_jpeg_encode_tables_restart']),
    'progressive': ({'progressive': True}, 'jpeg_progressive_ecd_bound',
                    ['nimg_jpeg_progressive_histogram', 'nimg_jpeg_optimal_tables', 'nimg_jpeg_encode_progressive']),
}
SUBSAMPLING = '4:2:0'


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


@pytest.mark.parametrize('ri', (0, 1))
@pytest.mark.parametrize('mode', list(MODES))
def test_library_calls_per_batch(dev, calls, monkeypatch, mode, ri):
    kw, bound, coding = MODES[mode]
    x = jpeg_cases.build(jpeg_cases.by_name('noise+smooth+constant+checker_16x24_q75_422'))[:2]              # n = 2 images of 16x24
    qtables = np.stack([jh.libjpeg_qtable(60, c).ravel() for c in (0, 1)])

    files = jh.encode_batch(x, 75, SUBSAMPLING, restart_interval=ri, **kw)
    assert _taken(calls) == ['nimg_jpeg_transform'] + coding
    jh.encode_batch(x, None, SUBSAMPLING, qtables=qtables, restart_interval=ri, **kw)
    assert _taken(calls) == ['nimg_jpeg_transform_tables'] + coding

    jh.compress_batch(x, 75, subsampling=SUBSAMPLING, restart_interval=ri, **kw)
    assert _taken(calls) == ['nimg_jpeg_transform'] + coding + ['nimg_jpeg_reconstruct']
    jh.compress_batch(x, None, subsampling=SUBSAMPLING, qtables=qtables, restart_interval=ri, **kw)
    assert _taken(calls) == ['nimg_jpeg_transform_tables'] + coding + ['nimg_jpeg_reconstruct_tables']

    baseline = jh.encode_batch(x, 75, SUBSAMPLING, restart_interval=ri)
    del calls[:]
    again = jh.transcode_batch(baseline, optimize=mode != 'plain', allow_restart=True, progressive=mode == 'progressive')
    assert _taken(calls) == ['nimg_jpeg_decode_restart'] + coding
    assert again == files

    # a first guess that is too small: the lengths say so, and exactly one more encode with what they ask for gives the same files
    monkeypatch.setattr(ops, bound, lambda *a: 16)
    assert jh.encode_batch(x, 75, SUBSAMPLING, restart_interval=ri, **kw) == files
    assert _taken(calls) == ['nimg_jpeg_transform'] + coding + coding[-1:]


# ---- (b) the shared checks ----------------------------------------------------------------------------------------------------------
def _tables(n_tables):
    return lambda dev: (torch.zeros((1, n_tables, 272), dtype=torch.uint8, device=dev),)


def _qtabs(dev):
    return (torch.ones((1, 3, 64), dtype=torch.int16, device=dev),)


# op -> (what it takes between the coefficients and h, w; behind h, w; the library's size of its workspace, None = it takes none)
COEF_OPS = {
    'jpeg_encode': (None, None, 'nimg_jpeg_encode_restart_workspace_bytes'),
    'jpeg_reconstruct': (None, lambda dev: (75,), 'nimg_jpeg_encode_restart_workspace_bytes'),
    'jpeg_reconstruct_items': (None, lambda dev: ([75],), 'nimg_jpeg_encode_restart_workspace_bytes'),
    'jpeg_reconstruct_tables': (None, _qtabs, 'nimg_jpeg_encode_restart_workspace_bytes'),
    'jpeg_histogram': (None, None, None),
    'jpeg_encode_tables': (_tables(4), None, 'nimg_jpeg_encode_tables_restart_workspace_bytes'),
    'jpeg_progressive_histogram': (None, None, None),
    'jpeg_encode_progressive': (_tables(10), None, 'nimg_jpeg_progressive_workspace_bytes'),
}


def _call(op, coef, h, w, dev, **kw):
    front, behind, _ = COEF_OPS[op]
    return getattr(ops, op)(coef, *(front(dev) if front else ()), h, w, *(behind(dev) if behind else ()), **kw)


@pytest.mark.parametrize('side', (8, 16))
@pytest.mark.parametrize('op', list(COEF_OPS))
def test_coefficient_ops_refuse(dev, calls, op, side):
    blocks = ops.jpeg_geometry(side, side, 1, 1)[0]
    good = torch.zeros((1, blocks, 64), dtype=torch.int16, device=dev)
    with pytest.raises(RuntimeError, match=op + ': coefficients torch.int32 .* do not match the geometry'):
        _call(op, good.int(), side, side, dev)
    if op != 'jpeg_progressive_histogram':                 # (test_gpu_jpegprog.py's test_arguments holds that one to its shape)
        with pytest.raises(RuntimeError, match=op + ': coefficients torch.int16 .* do not match the geometry'):
            _call(op, good[:, :-1].contiguous(), side, side, dev)
    size = COEF_OPS[op][2]
    if size is not None:
        need = int(getattr(_lib.load(), size)(1, side, side, 1, 1, 0))
        assert need > 1
        with pytest.raises(RuntimeError, match='workspace of {} bytes, {} needed'.format(need - 1, need)):
            _call(op, good, side, side, dev, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    assert calls == [], 'a refused call reached the library'


@pytest.mark.parametrize('op', ('jpeg_transform', 'jpeg_transform_items', 'jpeg_transform_tables'))
def test_transforms_refuse(dev, calls, op):
    second = {'jpeg_transform': 75, 'jpeg_transform_items': [75], 'jpeg_transform_tables': _qtabs(dev)[0]}[op]
    for x in (torch.zeros((1, 8, 8, 3), dtype=torch.float64, device=dev), torch.zeros((1, 16, 16, 4), dtype=torch.float32, device=dev)):
        with pytest.raises(RuntimeError, match=op + r' needs an \(n,h,w,3\) float32 or uint8 tensor'):
            getattr(ops, op)(x, second)
    assert calls == []


def test_progressive_encode_takes_an_empty_batch(dev):
    coef = torch.zeros((0, 12, 64), dtype=torch.int16, device=dev)
    tables = torch.zeros((0, 10, 272), dtype=torch.uint8, device=dev)
    out, lengths, status = ops.jpeg_encode_progressive(coef, tables, 16, 16)
    assert tuple(lengths.shape) == (0, 10) and lengths.dtype == torch.int32 and tuple(status.shape) == (0,)
