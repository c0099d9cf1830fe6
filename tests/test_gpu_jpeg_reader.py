"""Every kind of decode group in one call of the JPEG readers: two files each of baseline 4:2:0, the same geometry
with a restart interval, the same geometry progressive, grey-scale baseline, grey-scale progressive and 4:1:1, interleaved so that no
group's files stand next to each other.  The groups differ in what a file brings - six Huffman tables, two, or three per scan; three
quantisation tables or one; one segment or ten -, so a wrong offset into the uploaded segments, the table array or the quantisation
tables shows as wrong pixels of a later group.  Everything exact, against the golden pixels of the single-kind tests."""
import zlib

import numpy as np
import pytest
import torch

import jpeg_cases
import jpegdprog_cases
import jpeggrey_cases
import jpegprog_cases
import jpegrst_cases
import jpegsamp_cases
from neural_imaging_amd import _lib
from neural_imaging_amd.compression import jpeg_helpers as jh

pytestmark = pytest.mark.gpu

ALL = dict(allow_restart=True, allow_progressive=True, allow_grey=True, allow_sampling=True)
KINDS = ('baseline', 'restart', 'progressive', 'grey', 'grey progressive', '4:1:1')


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


def _crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff


def _kinds():
    """kind -> [(file, shape of its image, CRC32 of Pillow's pixels)] x 2, from the golden files of the single-kind tests."""
    colour = 'smooth+noise+half_13x21_q95_420'
    _, base, rgb = jpeg_cases.golden()[colour]
    rst = jpegrst_cases.golden()['noise+smooth_13x21_q75_420_ri1']
    prog, crcs = jpegprog_cases.golden()['g_' + colour], jpegdprog_cases.stored()[1]
    grey = jpeggrey_cases.golden()['flat+noise+mixed_20x27_q75_ri0']
    wide = [jpegsamp_cases.golden()[name] for name in ('noise_37x67_q30_411', 'mixed_37x67_q90_411')]
    return {
        'baseline': [(base[i], (13, 21, 3), _crc(rgb[i])) for i in (0, 1)],
        'restart': [(rst.files['plain'][i], (13, 21, 3), _crc(rst.rgb[i])) for i in (0, 1)],
        'progressive': [(prog[i], (13, 21, 3), crcs['g_{}|{}|std'.format(colour, i)]) for i in (0, 1)],
        'grey': [(grey.files['plain'][i], (20, 27, 1), _crc(grey.pixels[i])) for i in (1, 2)],
        'grey progressive': [(grey.files['prog'][i], (20, 27, 1), _crc(grey.pixels[i])) for i in (2, 1)],
        '4:1:1': [(g.files['plain'], (37, 67, 3), g.crcs[1]) for g in wide],
    }


def test_every_kind_of_group_in_one_call(dev, calls):
    kinds = _kinds()
    mixed = [kinds[k][i] for i in (0, 1) for k in KINDS]              # kind after kind, twice: input index = 6 * i + kind
    files = [f for f, _, _ in mixed]
    headers = [jh.parse_header(f, *[True] * 4) for f in files]
    assert [(hd.ncomp, hd.restart_interval, len(hd.scans)) for hd in headers[:6]] == [(3, 0, 0), (3, 1, 0), (3, 0, 10), (1, 0, 0), (1, 0, 6), (3, 0, 0)]
    assert (headers[5].hs, headers[5].vs) == (4, 1) and all((hd.hs, hd.vs) == (2, 2) for hd in headers[:3])

    del calls[:]
    images = jh.decode_batch(files, **ALL)
    decodes = ['nimg_jpeg_decode_restart', 'nimg_jpeg_decode_restart', 'nimg_jpeg_decode_progressive', 'nimg_jpeg_grey_decode',
               'nimg_jpeg_grey_decode_progressive', 'nimg_jpeg_sampling_decode']
    assert calls == decodes + ['nimg_jpeg_reconstruct_tables'] * 3 + ['nimg_jpeg_grey_reconstruct_tables'] * 2 + \
        ['nimg_jpeg_sampling_reconstruct_tables']                      # one decode and one reconstruction per group
    assert isinstance(images, list) and len(images) == 12
    for k, (y, (_, shape, crc)) in enumerate(zip(images, mixed)):
        assert y.dtype == np.uint8 and y.shape == shape and _crc(y) == crc, (k, KINDS[k % 6])

    alone = {k: [f for f, _, _ in kinds[k]] for k in KINDS}
    halves = jh.decode_batch(files, scale=2, **ALL)
    for j, k in enumerate(KINDS):
        want = jh.decode_batch(alone[k], scale=2, **ALL)
        assert want.shape == (2,) + jh.scaled_size(*kinds[k][0][1][:2], 2) + kinds[k][0][1][2:]
        assert np.array_equal(halves[j], want[0]) and np.array_equal(halves[6 + j], want[1]), k

    del calls[:]
    again = jh.transcode_batch(files, **ALL)
    assert [c for c in calls if 'decode' in c] == decodes and len(again) == 12
    for j, k in enumerate(KINDS):
        coef, qtables = jh.decode_coefficients(alone[k], **ALL)
        got, tables = jh.decode_coefficients([again[j], again[6 + j]], **ALL)
        assert np.array_equal(got, coef) and np.array_equal(tables, qtables), k
        for i in (j, 6 + j):                                            # written again as a baseline file of its interval and sampling
            hd = jh.parse_header(again[i], *[True] * 4)
            assert hd.scans == () and (hd.h, hd.w, hd.hs, hd.vs, hd.ncomp, hd.restart_interval) == \
                (headers[i].h, headers[i].w, headers[i].hs, headers[i].vs, headers[i].ncomp, headers[i].restart_interval), (i, k)
