"""The JPEG decoder on the host (no GPU): compression.jpeg_helpers.parse_header against the restatement's parser and its refusals;
the yardstick itself (jpeg_ref.parse + the tables of the file = Pillow's image); the sequential core of csrc/jpegd.h built into a
stand-alone program under AddressSanitizer and UBSan, on valid and damaged streams; and the Python model of the parallel algorithm
(tests/jpegd_ref.py) against that program."""
import importlib.util
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import jpeg_ref as ref
import jpegd_cases as cases
import jpegd_ref as dref
from neural_imaging_amd.compression import jpeg_helpers as jh


# ---- 1. parser --------------------------------------------------------------------------------------------------------------
def test_parse_header_equals_the_restatement():
    for f in cases.files():
        hd, info, head = jh.parse_header(f.data), ref.parse(f.data), dref.header(f.data)
        assert (hd.h, hd.w, hd.hs, hd.vs) == (info['h'], info['w'], info['hs'], info['vs']), f.name
        assert (hd.ecd_offset, hd.ecd_end) == (info['ecd_offset'], len(f.data) - 2), f.name
        assert hd.qtables.dtype == np.uint16 and hd.qtables.shape == (3, 64)
        for c in range(3):
            assert np.array_equal(hd.qtables[c], info['qtables'][head['q'][c]]), (f.name, c)
        assert list(hd.huffman) == head['tables'], f.name


def test_parse_header_reads_separate_chroma_tables():
    """Cb and Cr with tables of their own: three quantisation tables, six Huffman slots."""
    data = cases.by_name('mixed_24x32_444_qt-high').data
    head = dref.header(data)
    sof, sos = data.index(b'\xff\xc0'), data.index(b'\xff\xda')
    dqt = data.index(b'\xff\xdb')
    size = struct.unpack_from('>H', data, dqt + 2)[0]
    third = b'\xff\xdb\x00\x43\x02' + bytes(range(1, 65))
    dht = b''.join(b'\xff\xc4' + struct.pack('>H', 19 + len(s)) + bytes([ident]) + c + s
                   for ident, (c, s) in ((0x02, head['tables'][0]), (0x12, head['tables'][1])))
    edited = bytearray(data[:dqt + 2 + size] + third + dht + data[dqt + 2 + size:])
    shift = len(third) + len(dht)
    edited[sof + shift + 4 + 6 + 8] = 2                      # Cr: quantisation table 2
    edited[sos + shift + 4 + 6] = 0x22                       # Cr: Huffman tables 2 / 2
    hd = jh.parse_header(bytes(edited))
    natural = np.zeros(64, np.int64)
    natural[ref.ZZ] = np.arange(1, 65)
    assert hd.qtables[2].tolist() == natural.tolist()
    assert not np.array_equal(hd.qtables[1], hd.qtables[2])
    assert hd.huffman[4:] == (head['tables'][0], head['tables'][1]) and hd.huffman[2:4] == tuple(head['tables'][2:4])


def _edit(data, marker, offset, value):
    """The file with byte `offset` of the body of its first `marker` segment replaced."""
    at = data.index(marker) + 4 + offset
    return data[:at] + bytes([value]) + data[at + 1:]


def _refusals():
    base = cases.by_name('smooth_13x21_q75_420/0').data              # a file written with the Annex K tables
    sos, dht = base.index(b'\xff\xda'), base.index(b'\xff\xc4')
    dht_size = struct.unpack_from('>H', base, dht + 2)[0]
    return [
        ('progressive', base.replace(b'\xff\xc0', b'\xff\xc2', 1)),
        ('extended sequential', base.replace(b'\xff\xc0', b'\xff\xc1', 1)),
        ('12-bit samples', _edit(base, b'\xff\xc0', 0, 12)),
        ('16-bit quantisation', _edit(base, b'\xff\xdb', 0, 0x10)),
        ('sampling factors', _edit(base, b'\xff\xc0', 7, 0x12)),
        ('sampling factors', _edit(base, b'\xff\xc0', 10, 0x21)),
        ('sampling factors', _edit(base, b'\xff\xc0', 7, 0x41)),
        ('restart interval', base[:sos] + b'\xff\xdd\x00\x04\x00\x08' + base[sos:]),
        ('missing Huffman table', base[:dht] + base[dht + 2 + dht_size:]),
        ('missing quantisation table', _edit(base, b'\xff\xc0', 11, 3)),
        ('not a baseline scan', _edit(base, b'\xff\xda', 8, 5)),
        ('not a baseline scan', _edit(base, b'\xff\xda', 7, 1)),
        ('not a baseline scan', _edit(base, b'\xff\xda', 9, 0x10)),
        ('no EOI', base[:-2]),
        ('no EOI', base[:-1]),
        ('several scans', base[:-2] + base[sos:]),
        ('restart marker', base[:-2] + b'\xff\xd0' + base[-2:]),
        ('no SOI', base[2:]),
        ('no frame header', base[:base.index(b'\xff\xc0')] + base[dht:]),
        ('truncated', base[:sos + 3]),
    ]


@pytest.mark.parametrize('reason,data', _refusals(), ids=['{}-{}'.format(i, r[0]) for i, r in enumerate(_refusals())])
def test_parse_header_refuses(reason, data):
    with pytest.raises(ValueError, match=reason):
        jh.parse_header(data)
    with pytest.raises(ValueError, match=reason):                    # refused before anything reaches a device
        jh.decode_batch([data], device='no device is touched')


def test_parse_header_refuses_component_counts():
    """Grey-scale, CMYK and non-interleaved files, made from a golden header."""
    base = cases.by_name('smooth_13x21_q75_420/0').data
    sof, sos = base.index(b'\xff\xc0'), base.index(b'\xff\xda')
    grey = base[:sof] + b'\xff\xc0\x00\x0b' + base[sof + 4:sof + 9] + b'\x01\x01\x11\x00' + base[sof + 19:]
    cmyk = base[:sof] + b'\xff\xc0\x00\x14' + base[sof + 4:sof + 9] + b'\x04' + base[sof + 10:sof + 19] + b'\x04\x11\x01' + base[sof + 19:]
    single = base[:sos] + b'\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00' + base[sos + 14:]
    for reason, data in (('grey-scale', grey), ('CMYK', cmyk), ('non-interleaved', single)):
        with pytest.raises(ValueError, match=reason):
            jh.parse_header(data)


def test_parse_header_refuses_pillow_files():
    Image = pytest.importorskip('PIL.Image')
    img = cases.foreign_image(cases.FOREIGN[0])

    def save(image, **args):
        buf = io.BytesIO()
        image.save(buf, format='JPEG', **args)
        return buf.getvalue()

    for reason, data in (('progressive', save(Image.fromarray(img), progressive=True)),
                         ('grey-scale', save(Image.fromarray(img[..., 0]))),
                         ('CMYK', save(Image.fromarray(img).convert('CMYK'))),
                         ('restart interval', save(Image.fromarray(img), restart_marker_blocks=2))):
        with pytest.raises(ValueError, match=reason):
            jh.parse_header(data)
    with_comment = save(Image.fromarray(img), comment=b'skipped', optimize=True)
    assert b'\xff\xfe' in with_comment and jh.parse_header(with_comment).h == img.shape[0]


def test_yardstick_equals_pillow():
    """jpeg_ref.parse + the tables of the file + jpeg_ref's inverse transform = Pillow's decode, on every golden file."""
    for f in cases.files():
        assert np.array_equal(dref.decode_u8(f.data), f.rgb), f.name


def test_golden_files_are_pillows():
    Image = pytest.importorskip('PIL.Image')
    spec = importlib.util.spec_from_file_location('make_jpegd_golden', os.path.join(os.path.dirname(cases.GOLDEN), 'make_jpegd_golden.py'))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    for case, f in zip(cases.FOREIGN, cases.foreign_files()):
        data, rgb = make.pillow(case)
        assert data == f.data and np.array_equal(rgb, f.rgb), case.name
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(f.data)).convert('RGB')), f.rgb)


def test_golden_files_reach_the_foreign_paths():
    names = [f.name for f in cases.foreign_files()]
    assert names == [c.name for c in cases.FOREIGN]
    annex_k = [bytes(ref.HUFF[t][0]) for t in (0x00, 0x10, 0x01, 0x11)]
    optimised = [f for f in cases.foreign_files() if [t[0] for t in dref.header(f.data)['tables'][:4]] != annex_k]
    assert len(optimised) >= 18
    assert max(int(q.max()) for f in cases.foreign_files() for q in ref.parse(f.data)['qtables'].values()) == 255
    stuffed = cases.by_name('noise_16x24_444_q100_opt')
    assert b'\xff\x00' in cases.stream_of(stuffed).ecd
    # the category limits of the decoder: a DC difference of category 11, an AC value of category 10 (4:4:4: raster = scan order)
    luma = {c: ref.parse(cases.by_name('{}_16x16_444_q100_opt'.format(c)).data)['coefs'][0].astype(np.int64) for c in ('half', 'checker')}
    assert np.abs(np.diff(luma['half'][..., 0].reshape(-1), prepend=0)).max() >= 1024
    assert np.abs(luma['checker'][..., 1:]).max() >= 512


# ---- 2. the sequential core under sanitizers, as a stand-alone program ------------------------------------------------------------
@pytest.fixture(scope='module')
def sanitized():
    try:                                                             # no compiler at all is host_program's assertion: a failure
        return cases.host_program(True)
    except subprocess.CalledProcessError as e:
        pytest.fail('the host program does not build with -fsanitize=address,undefined:\n' + e.stdout.decode())


@pytest.fixture(scope='module')
def valid_results(sanitized):
    results, done = cases.host_results(cases.valid_streams(), sanitize=True)
    assert done.returncode == 0 and done.stderr == b'', done.stderr.decode()[-4000:]
    return results


def test_host_program_decodes_every_golden_file(valid_results):
    for k, f in enumerate(cases.files()):
        want = ref.flat_coefficients(dref.real_coefficients(ref.parse(f.data)))
        for setting in cases.SETTINGS:
            r = valid_results[(k, setting)]
            assert r.status == 0, (f.name, setting, r.status)
            assert np.array_equal(r.coef, want), (f.name, setting)
            assert r.rounds <= r.subsequences, (f.name, setting)
            if setting == 0:
                assert r.subsequences == 1 and r.rounds == 0
    assert max(r.rounds for r in valid_results.values()) > 100         # long blocks over 32-bit subsequences: rounds do repeat


def test_host_program_survives_damaged_streams(sanitized):
    streams = cases.damaged_streams()
    kinds = [s.name.split('|')[1].rstrip('0123456789') for s in streams]
    assert (kinds.count('flip'), kinds.count('random'), kinds.count('allff')) == (200, 20, 1) and kinds.count('cut') > 2 * len(cases.files())
    results, done = cases.host_results(streams, sanitize=True)
    assert done.returncode == 0 and done.stderr == b'', done.stderr.decode()[-4000:]
    assert len(results) == len(streams) * len(cases.SETTINGS)
    for k, s in enumerate(streams):
        blocks = len(results[(k, 0)].coef) // 64
        for setting in cases.SETTINGS:
            r = results[(k, setting)]
            assert r.status != 0 or len(r.coef) == 64 * blocks, s.name      # a status bit, or a full coefficient tensor
            assert r.rounds <= r.subsequences, (s.name, setting)
            assert r.status == results[(k, 0)].status, (s.name, setting)    # the damage reads the same however the stream is cut
            if r.status == 0:
                assert np.array_equal(r.coef, results[(k, 0)].coef), (s.name, setting)
    assert sum(results[(k, 0)].status != 0 for k in range(len(streams))) > 200


# ---- 3. the Python model ------------------------------------------------------------------------------------------------------
def test_model_equals_the_host_program(valid_results):
    for k, (f, s) in enumerate(zip(cases.files(), cases.valid_streams())):
        model = dref.Model(s.h, s.w, s.hs, s.vs, dref.header(f.data)['tables'], s.ecd)
        for setting in cases.SETTINGS:
            coef, status, rounds, subsequences = model.run(setting)
            r = valid_results[(k, setting)]
            assert (status, rounds, subsequences) == (r.status, r.rounds, r.subsequences), (f.name, setting)
            assert np.array_equal(coef, r.coef), (f.name, setting)
